// The three operators an OpenCLIP text tower needs beside the generic GEMMs, pmhip_layernorm, pmhip_embed_rows and pmhip_add_rows
// (DESIGN.md section 4zl): causal self-attention, the head split of a projection that already carries its bias, and the two GELUs.
// The attention kernel has the structure of attention_relbias_kernel (t5ops.hip): one wave per 16 query rows of one (image, head),
// no LDS and no barrier.  The row kernels are one pass with 16-byte reads.
#include <math.h>

#include "attn_wave16.h"
#include "common.h"

namespace {

constexpr int THREADS = 256;

// ------------------------------------------------------------------------------------------------
// Causal self-attention: query q attends to the keys [0, q].  The wave of the queries [q0, q0 + 16) walks the keys [0, n),
// n = min(L, q0 + 16), in blocks of KB = 32 (bf16) / 16 (f32) with an exact running maximum (fragment maps: attn_wave16.h).  Blocks
// wholly above the diagonal are never visited; K rows >= n are never read (the row index is clamped to n - 1); a key k > q gets the
// score -inf by a select, so whatever its K row holds reaches nothing, and its probability is exactly 0.
// P V in two parts, because the matrix core shares its V^T operand among the 16 queries and 0 * NaN is NaN:
//   keys < q0            every query of the tile may see them: O^T += V^T . P^T on the matrix core, with the V^T elements of keys
//                        >= q0 replaced by 0 as they are loaded (P rounded to bf16 once in bf16 mode, as in the relbias kernel)
//   keys [q0, q0 + 16)   the diagonal tile, on the vector ALU: a lane gathers its query's 16 probabilities from the lanes {c, c+16,
//                        c+32, c+48} by row / half swaps and takes V^T[dim, key] with a select `key <= q ? value : 0` (a group of 4
//                        keys is read only when its first key is allowed).  P stays f32 here.  Up to 256 multiply-adds per lane,
//                        once per wave, behind the key walk.
// So row q depends on no K row and no V^T column > q, NaN included, nor on [L, L_pad).  Queries >= L of the last tile repeat row
// L - 1 and are not stored.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load_keys4(const float* p, float (&v)[4]) {
    const float4 x = *reinterpret_cast<const float4*>(p);
    v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
}
__device__ __forceinline__ void load_keys4(const bf16_t* p, float (&v)[4]) {
    const uint2 x = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(x.x << 16), v[1] = __uint_as_float(x.x & 0xffff0000u);
    v[2] = __uint_as_float(x.y << 16), v[3] = __uint_as_float(x.y & 0xffff0000u);
}

template <typename T>
__global__ __launch_bounds__(64) void attention_causal_kernel(const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ Vt,
                                                              T* __restrict__ out, int ldo, int heads, int L, int L_pad) {
    constexpr int E = Mma<T>::kElemsPerChunk;       // elements of a 16-byte chunk: 8 (bf16) / 4 (f32)
    constexpr int NT = E / 4;                       // 16-key tiles of a block
    constexpr int KB = 16 * NT;                     // keys of a block
    constexpr int DS = 64 / (4 * E);                // chunks of a 64-wide Q / K row per lane
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15;
    const int b = blockIdx.z, h = blockIdx.y, q0 = blockIdx.x * 16;
    const int n = min(L, q0 + 16);                  // the tile's last allowed key is n - 1
    const size_t bh = (size_t)b * heads + h;
    const T* Qp = Q + bh * L * 64;
    const T* Kp = K + bh * L_pad * 64;
    const T* Vp = Vt + bh * 64 * L_pad;
    const int qc = min(q0 + c, L - 1);

    uint4 qf[DS];
#pragma unroll
    for (int s = 0; s < DS; ++s) qf[s] = *reinterpret_cast<const uint4*>(Qp + (size_t)qc * 64 + s * 4 * E + g * E);

    f32x4_t o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;
    f32x4_t pd = f32x4_t{0.f, 0.f, 0.f, 0.f};

    for (int k0 = 0; k0 < n; k0 += KB) {
        f32x4_t sc[NT];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int kb = k0 + 16 * t;
            if (kb < n) {                           // wave-uniform: the second tile of a bf16 block may lie above the diagonal
                const int kr = min(kb + c, n - 1);
                f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < DS; ++s) {
                    const uint4 kf = *reinterpret_cast<const uint4*>(Kp + (size_t)kr * 64 + s * 4 * E + g * E);
                    Mma<T>::run(acc, kf, qf[s]);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sv = kb + 4 * g + r <= qc ? acc[r] : -INFINITY;
                    sc[t][r] = sv;
                    mx = fmaxf(mx, sv);
                }
            } else {
                sc[t] = f32x4_t{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
            }
        }
        mx = group4_max(mx);
        const float m_new = fmaxf(m, mx);           // finite from the first block on: key 0 is allowed for every query
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
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) o[dt][r] *= alpha;
        if (k0 < q0) {                              // keys every query of the tile sees: the matrix core
            const uint4 pf = pack_probs<T>(sc);
            const bool full = k0 + KB <= q0;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) Mma<T>::run(o[dt], load_vt(Vp + (size_t)(16 * dt + c) * L_pad, k0, g, q0, full), pf);
        }
        pd = (NT == 2 && q0 > k0) ? sc[NT - 1] : sc[0];       // of the last block: the diagonal tile's probabilities
    }
    // the diagonal tile (it lies in the last block walked): the vector ALU, after the loop so that its addresses are not kept alive
    // through the key walk
    {
        f32x4_t pj[4];                              // pj[j][r]: the lane's query against key q0 + 4 (g ^ j) + r
        pj[0] = pd;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pj[1][r] = __uint_as_float(other16(__float_as_uint(pd[r]), lane));
            pj[2][r] = __uint_as_float(other32(__float_as_uint(pd[r]), lane));
            pj[3][r] = __uint_as_float(other16(__float_as_uint(pj[2][r]), lane));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ks = q0 + 4 * (g ^ j);
            if (ks <= qc) {                         // ks <= qc < L and ks, L_pad multiples of 4: the 4 keys lie inside the row
                const T* vb = Vp + (size_t)(4 * g) * L_pad + ks;
#pragma unroll
                for (int dt = 0; dt < 4; ++dt)
#pragma unroll
                    for (int rr = 0; rr < 4; ++rr) {
                        float v[4];
                        load_keys4(vb + (16 * dt + rr) * L_pad, v);     // (16 dt + rr) L_pad < 2^26: a wave-uniform 32-bit offset
#pragma unroll
                        for (int r = 0; r < 4; ++r) o[dt][rr] = fmaf(pj[j][r], ks + r <= qc ? v[r] : 0.f, o[dt][rr]);
                    }
            }
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
int launch_causal(const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int L, int L_pad, hipStream_t s) {
    dim3 grid(ceil_div(L, 16), heads, B), block(64);
    PmTimer tm(FAM_ATTENTION, s);
    hipLaunchKernelGGL((attention_causal_kernel<T>), grid, block, 0, s, reinterpret_cast<const T*>(Q), reinterpret_cast<const T*>(K),
                       reinterpret_cast<const T*>(Vt), reinterpret_cast<T*>(out), ldo, heads, L, L_pad);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

// ------------------------------------------------------------------------------------------------
// Head split of a projection that is already computed (bias included) in f32: part p = the columns [p * heads * 64, (p + 1) * heads
// * 64) of U, written as pmhip_gemm_heads writes it and rounded once.  One thread = 4 consecutive columns of one row (one 16-byte
// read); Q and K are one 4-element store, V^T four scalar stores down a column.  The padding [tokens, tokens_pad) is not touched.
// ------------------------------------------------------------------------------------------------
struct SplitArgs {
    const float* u;
    void* outs[3];
    int kinds[3];
    int ldu, M, heads, tokens, tokens_pad, nparts;
    float q_scale;
};

template <typename T>
__global__ __launch_bounds__(THREADS) void split_heads_kernel(SplitArgs p) {
    const int inner4 = p.heads * 16, n4 = p.nparts * inner4;
    const size_t idx = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= (size_t)p.M * n4) return;
    const int m = (int)(idx / n4), c4 = (int)(idx % n4);
    const int part = c4 / inner4, hc = (c4 % inner4) * 4, h = hc >> 6, d = hc & 63;
    const float4 v = *reinterpret_cast<const float4*>(p.u + (size_t)m * p.ldu + (size_t)part * inner4 * 4 + hc);
    const int b = m / p.tokens, t = m % p.tokens;
    const size_t bh = (size_t)b * p.heads + h;
    T* o = reinterpret_cast<T*>(p.outs[part]);
    const int kind = p.kinds[part];
    if (kind == PMHIP_PART_Q) {
        const float s = p.q_scale;
        store4(o + (bh * p.tokens + t) * 64 + d, __fmul_rn(v.x, s), __fmul_rn(v.y, s), __fmul_rn(v.z, s), __fmul_rn(v.w, s));
    } else if (kind == PMHIP_PART_K) {
        store4(o + (bh * p.tokens_pad + t) * 64 + d, v.x, v.y, v.z, v.w);
    } else {
        T* col = o + (bh * 64 + d) * p.tokens_pad + t;
        col[0] = from_f32<T>(v.x);
        col[(size_t)p.tokens_pad] = from_f32<T>(v.y);
        col[2 * (size_t)p.tokens_pad] = from_f32<T>(v.z);
        col[3 * (size_t)p.tokens_pad] = from_f32<T>(v.w);
    }
}

// ------------------------------------------------------------------------------------------------
// The two GELUs of OpenCLIP's text towers on the f32 output of the c_fc GEMM.  One thread = 4 consecutive columns.
//   erf    nn.GELU(): 0.5 x (1 + erf(x / sqrt 2)) evaluated as 0.5 x erfc(-x sqrt(0.5)) -- the same function without the cancellation
//          of 1 + erf at negative x.  0.5 x is exact and erfc is in [0, 2]: finite x gives a finite result.
//   quick  QuickGELU: x sigmoid(1.702 x) evaluated as x / (1 + exp(-1.702 x)); where the exponential is 0 or inf (the product
//          included) the quotient is x or -0: finite x gives a finite result.
// ------------------------------------------------------------------------------------------------
template <int KIND> __device__ __forceinline__ float gelu_of(float x);
template <> __device__ __forceinline__ float gelu_of<0>(float x) { return (0.5f * x) * erfcf(-x * 0.70710678118654752f); }
template <> __device__ __forceinline__ float gelu_of<1>(float x) { return x / (1.0f + expf(-1.702f * x)); }

template <typename OutT, int KIND>
__global__ __launch_bounds__(THREADS) void gelu_kernel(const float* __restrict__ u, int ldu, OutT* __restrict__ out, int ldo, int M, int F) {
    const int f4 = F / 4;
    const size_t idx = (size_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= (size_t)M * f4) return;
    const size_t m = idx / f4;
    const int j = (int)(idx % f4) * 4;
    const float4 a = *reinterpret_cast<const float4*>(u + m * ldu + j);
    store4(out + m * ldo + j, gelu_of<KIND>(a.x), gelu_of<KIND>(a.y), gelu_of<KIND>(a.z), gelu_of<KIND>(a.w));
}

template <typename OutT>
void launch_gelu(const float* u, int ldu, void* out, int ldo, int M, int F, int kind, dim3 grid, hipStream_t s) {
    OutT* o = reinterpret_cast<OutT*>(out);
    if (kind == 0) hipLaunchKernelGGL((gelu_kernel<OutT, 0>), grid, dim3(THREADS), 0, s, u, ldu, o, ldo, M, F);
    else hipLaunchKernelGGL((gelu_kernel<OutT, 1>), grid, dim3(THREADS), 0, s, u, ldu, o, ldo, M, F);
}

}  // namespace

extern "C" int pmhip_attention_causal(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int L,
                                      int L_pad, pmhip_stream stream) {
    PM_REQUIRE(dtype == PMHIP_F32 || dtype == PMHIP_BF16, "attention_causal: bad dtype %d", dtype);
    PM_REQUIRE(Q && K && Vt && out, "attention_causal: null pointer (Q, K, Vt or out)");
    PM_REQUIRE(B > 0 && B <= 65535 && heads > 0 && heads <= 65535, "attention_causal: B=%d and heads=%d must be in [1, 65535]", B, heads);
    PM_REQUIRE(L >= 1 && L <= (1 << 20), "attention_causal: L=%d must be in [1, 2^20]", L);
    PM_REQUIRE(L_pad >= L && L_pad % 4 == 0 && L_pad <= (1 << 24), "attention_causal: L_pad=%d must be a multiple of 4 in [L=%d, 2^24]", L_pad, L);
    PM_REQUIRE(ldo >= heads * 64 && ldo % 4 == 0, "attention_causal: ldo=%d must be a multiple of 4 >= heads*64=%d", ldo, heads * 64);
    PM_REQUIRE(pm_aligned(16, {Q, K, Vt}) && pm_aligned(dtype == PMHIP_F32 ? 16 : 8, {out}),
               "attention_causal: Q, K, Vt must be 16-byte aligned and out 4-element aligned");
    hipStream_t s = (hipStream_t)stream;
    if (dtype == PMHIP_F32) return launch_causal<float>(Q, K, Vt, out, ldo, B, heads, L, L_pad, s);
    return launch_causal<bf16_t>(Q, K, Vt, out, ldo, B, heads, L, L_pad, s);
}

extern "C" int pmhip_split_heads(int dtype, const float* U, int ldu, int M, int heads, int tokens, int tokens_pad, int nparts,
                                 const int* part_kinds_host, void* const* part_outs_host, float q_scale, pmhip_stream stream) {
    PM_REQUIRE(dtype == PMHIP_F32 || dtype == PMHIP_BF16, "split_heads: bad dtype %d", dtype);
    PM_REQUIRE(U, "split_heads: U is NULL");
    PM_REQUIRE(nparts >= 1 && nparts <= 3 && part_kinds_host && part_outs_host, "split_heads: nparts=%d must be 1..3 with both host arrays", nparts);
    PM_REQUIRE(heads > 0 && heads <= (1 << 16), "split_heads: heads=%d must be in [1, 65536]", heads);
    PM_REQUIRE(tokens > 0 && tokens_pad >= tokens && M > 0 && M % tokens == 0,
               "split_heads: bad token geometry M=%d tokens=%d tokens_pad=%d (M a multiple of tokens, tokens_pad >= tokens)", M, tokens, tokens_pad);
    PM_REQUIRE((long long)nparts * heads * 64 <= ldu && ldu % 4 == 0, "split_heads: ldu=%d must be a multiple of 4 >= nparts*heads*64=%lld", ldu,
               (long long)nparts * heads * 64);
    PM_REQUIRE(pm_aligned(16, {U}), "split_heads: U must be 16-byte aligned");
    SplitArgs p{};
    p.u = U; p.ldu = ldu; p.M = M; p.heads = heads; p.tokens = tokens; p.tokens_pad = tokens_pad; p.nparts = nparts; p.q_scale = q_scale;
    for (int i = 0; i < nparts; ++i) {
        PM_REQUIRE(part_kinds_host[i] >= 0 && part_kinds_host[i] <= 2, "split_heads: part %d has kind %d (0 Q, 1 K, 2 V)", i, part_kinds_host[i]);
        PM_REQUIRE(part_outs_host[i] && pm_aligned(16, {part_outs_host[i]}), "split_heads: the output of part %d must be a 16-byte aligned pointer", i);
        p.outs[i] = part_outs_host[i]; p.kinds[i] = part_kinds_host[i];
    }
    const size_t total = (size_t)M * nparts * heads * 16;
    PM_REQUIRE(total <= 0x7fffffffull * THREADS, "split_heads: M*nparts*heads too large");
    hipStream_t s = (hipStream_t)stream;
    dim3 grid((unsigned)((total + THREADS - 1) / THREADS)), block(THREADS);
    PmTimer tm(FAM_ROWOPS, s);
    if (dtype == PMHIP_F32) hipLaunchKernelGGL(split_heads_kernel<float>, grid, block, 0, s, p);
    else hipLaunchKernelGGL(split_heads_kernel<bf16_t>, grid, block, 0, s, p);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

extern "C" int pmhip_gelu(const float* u, int ldu, void* out, int ldo, int out_dtype, int M, int F, int kind, pmhip_stream stream) {
    PM_REQUIRE(u && out, "gelu: null pointer");
    PM_REQUIRE(out_dtype == PMHIP_F32 || out_dtype == PMHIP_BF16, "gelu: bad out_dtype %d", out_dtype);
    PM_REQUIRE(kind == 0 || kind == 1, "gelu: bad kind %d (0 = erf, 1 = quick)", kind);
    PM_REQUIRE(M > 0 && F > 0 && F % 4 == 0, "gelu: bad shape M=%d F=%d (F must be a multiple of 4)", M, F);
    PM_REQUIRE(ldu >= F && ldu % 4 == 0, "gelu: ldu=%d must be a multiple of 4 >= F=%d", ldu, F);
    PM_REQUIRE(ldo >= F && ldo % 4 == 0, "gelu: ldo=%d must be a multiple of 4 >= F=%d", ldo, F);
    PM_REQUIRE(pm_aligned(16, {u}) && pm_aligned(out_dtype == PMHIP_F32 ? 16 : 8, {out}), "gelu: u / out must be 16-byte / 4-element aligned");
    hipStream_t s = (hipStream_t)stream;
    const size_t total = (size_t)M * (F / 4);
    PM_REQUIRE(total <= 0x7fffffffull * THREADS, "gelu: M*F too large");
    dim3 grid((unsigned)((total + THREADS - 1) / THREADS));
    PmTimer tm(FAM_ROWOPS, s);
    if (out_dtype == PMHIP_F32) launch_gelu<float>(u, ldu, out, ldo, M, F, kind, grid, s);
    else launch_gelu<bf16_t>(u, ldu, out, ldo, M, F, kind, grid, s);
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}
