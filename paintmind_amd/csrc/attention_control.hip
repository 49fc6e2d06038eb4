// Cross-attention control: the edited pass of a prompt-to-prompt pair attends with probabilities blended from the
// source pass's.  Per pair b and head h, over the target keys j < nt (the pair's target length):
//
//   ps = softmax over k < ns of Qs Ks^T            pt = softmax over j < nt of Qt Kt^T
//   m = row_map[b, j];  has = 0 <= m < ns and blend[b, j] != 0
//   P[q, j] = gain[b, j] * (has ? (1 - blend[b, j]) * pt[q, j] + blend[b, j] * ps[q, m] : pt[q, j])
//   O[b, q, h * dh : (h + 1) * dh] = sum_j P[q, j] * V[j, :]                     (no renormalisation)
//
// The flash kernels never hold a row of P, so neither pass's probabilities exist anywhere; this file recomputes both, in the two-pass
// structure of attention_maps.hip and from the shared pieces of attention_probs.h (which holds THE definition of `has` and P).  A workgroup owns one (pair, head) and 64 queries:
//   pass 1 : the maximum m and the sum l of every query row of BOTH softmaxes, (m, 1 / l) kept in registers
//   pass 2 : walk the target keys, recompute Qt . Kt[j] and Qs . Ks[row_map[j]] (the Ks ROWS are gathered through row_map; no P is
//            stored), blend, scale, accumulate P . V
// so registers do not depend on the context, there is no LDS, every element of O is written by exactly one thread once, and there
// are no atomics.
//   attention_control_mfma_kernel  bf16, dim_head 64.  S^T = K Q^T by v_mfma_f32_16x16x32_bf16 (keys on the rows): a lane then holds
//                                  the scores of ONE query (lane & 15) and of keys 4 g + r, which is already the operand layout of the
//                                  P . V MFMA once the k index of a 32-key chunk is read as (16 t + 4 g + r); V^T is loaded in the same
//                                  order, so P never crosses lanes.  P is rounded to bf16 for that MFMA, as the product kernel does.
//   attention_control_valu_kernel  everything else (fp32, dim_head != 64), in the manner of attention_dh.hip: 4 lanes share a query,
//                                  each owning dh / 4 dims of q and of the output; P stays f32.
// Select, never arithmetic: a target key at or behind nt contributes through no operation: its K row is not read; its V^T column is
// not read in the vector-ALU kernel, and in the MFMA kernel it is read only inside the 8-byte group of 4 keys that straddles nt (in
// bounds: Lt_pad is a multiple of 4) and zeroed by a select; where `has` is false the gathered row is row 0 of the pair's
// own Ks in the MFMA kernel (any lane must feed the matrix core something) and nothing in the other, and its score is dropped by a
// select; source rows at or behind ns are never read.
#include "attention_probs.h"

namespace {

struct CtlParams {
    void* out;
    int ldo, heads, Nq, Ls, Lsp, Lt, Ltp;
    PairControl ctl;
    const int* lens_s;                  // [B] or NULL
    const int* lens_t;                  // [B] or NULL
};

template <bool EXP2>
__global__ __launch_bounds__(256) void attention_control_mfma_kernel(const bf16_t* __restrict__ Qs, const bf16_t* __restrict__ Ks,
                                                                     const bf16_t* __restrict__ Qt, const bf16_t* __restrict__ Kt,
                                                                     const bf16_t* __restrict__ Vt, CtlParams p) {
    const int bh = blockIdx.y, b = bh / p.heads, h = bh % p.heads;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const int Nq = p.Nq;
    const int ns = prob_len(p.lens_s, b, p.Ls), nt = prob_len(p.lens_t, b, p.Lt);
    const int q0 = blockIdx.x * 64 + wave * 16;
    const int qi = q0 + col;                                    // this lane's query: every score and every output it holds
    const int qa = qi < Nq ? qi : Nq - 1;                       // (rows past the end: a copy, never stored)
    // 8 dims per lane and MFMA: [8 g, 8 g + 8) and [32 + 8 g, 32 + 8 g + 8), the same for both operands
    uint4 qs0, qs1, qt0, qt1;
    {
        const uint4* a = reinterpret_cast<const uint4*>(Qs + ((size_t)bh * Nq + qa) * 64 + g * 8);
        const uint4* c = reinterpret_cast<const uint4*>(Qt + ((size_t)bh * Nq + qa) * 64 + g * 8);
        qs0 = a[0]; qs1 = a[4]; qt0 = c[0]; qt1 = c[4];
    }
    const bf16_t* ksb = Ks + (size_t)bh * p.Lsp * 64 + g * 8;
    const bf16_t* ktb = Kt + (size_t)bh * p.Ltp * 64 + g * 8;
    float ms, is, mt, it;
    kq_stats<EXP2>(ksb, ns, qs0, qs1, col, g, ms, is);
    kq_stats<EXP2>(ktb, nt, qt0, qt1, col, g, mt, it);

    f32x4_t o[4];                                               // o[db][r] = O[query col][16 db + 4 g + r]
#pragma unroll
    for (int db = 0; db < 4; ++db) o[db] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const bf16_t* vtb = Vt + ((size_t)bh * 64 + col) * p.Ltp;   // V^T row (16 db + col) is vtb + 16 db * Ltp

    for (int j0 = 0; j0 < nt; j0 += 32) {
        float pr[8];                                            // P[query col][j0 + 16 t + 4 g + r] at 4 t + r
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int jb = j0 + 16 * t;
#pragma unroll
            for (int r = 0; r < 4; ++r) pr[4 * t + r] = 0.f;
            if (jb >= nt) continue;                             // (workgroup-uniform)
            const int kj = jb + col;
            const f32x4_t st = kq_scores(ktb, kj < nt ? kj : nt - 1, qt0, qt1);
            f32x4_t ss = {0.f, 0.f, 0.f, 0.f};
            PM_KQ_GATHER(ss, p.ctl, p.Lt, b, kj, nt, ns, ksb, qs0, qs1);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = jb + 4 * g + r;
                if (j < nt) {
                    const PairKey k = pair_key(p.ctl, p.Lt, b, j, ns);
                    const float pt = prob_exp<EXP2>(st[r] - mt) * it;
                    const float ps = k.has ? prob_exp<EXP2>(ss[r] - ms) * is : 0.f;
                    pr[4 * t + r] = pair_mix(k, pt, ps);
                }
            }
        }
        const uint4 pf = make_uint4(pack_bf16x2(pr[0], pr[1]), pack_bf16x2(pr[2], pr[3]), pack_bf16x2(pr[4], pr[5]), pack_bf16x2(pr[6], pr[7]));
        // V^T in the same k order: keys j0 + 4 g + {0..3} and j0 + 16 + 4 g + {0..3}; a key at or behind nt becomes 0 by a select
        const int n0 = nt - (j0 + 4 * g), n1 = n0 - 16;         // how many of each group of 4 take part
        auto keep = [](uint2 v, int n) -> uint2 {
            if (n >= 4) return v;
            v.y = n >= 3 ? v.y & 0x0000FFFFu : 0u;
            v.x = n >= 2 ? v.x : v.x & 0x0000FFFFu;
            return v;
        };
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const bf16_t* vp = vtb + (size_t)(16 * db) * p.Ltp + j0 + 4 * g;
            uint2 v0 = make_uint2(0u, 0u), v1 = make_uint2(0u, 0u);
            if (n0 > 0) v0 = keep(*reinterpret_cast<const uint2*>(vp), n0);
            if (n1 > 0) v1 = keep(*reinterpret_cast<const uint2*>(vp + 16), n1);
            Mma<bf16_t>::run(o[db], make_uint4(v0.x, v0.y, v1.x, v1.y), pf);
        }
    }
    if (qi < Nq) {
        bf16_t* op = reinterpret_cast<bf16_t*>(p.out) + ((size_t)b * Nq + qi) * p.ldo + h * 64 + 4 * g;
#pragma unroll
        for (int db = 0; db < 4; ++db) store4(op + 16 * db, o[db][0], o[db][1], o[db][2], o[db][3]);
    }
}

// DPL = dims per lane = dh / 4
template <typename T, int DPL, bool EXP2>
__global__ __launch_bounds__(256) void attention_control_valu_kernel(const T* __restrict__ Qs, const T* __restrict__ Ks,
                                                                     const T* __restrict__ Qt, const T* __restrict__ Kt,
                                                                     const T* __restrict__ Vt, CtlParams p) {
    constexpr int DH = DPL * 4;
    const int bh = blockIdx.y, b = bh / p.heads, h = bh % p.heads;
    const int Nq = p.Nq;
    const int ns = prob_len(p.lens_s, b, p.Ls), nt = prob_len(p.lens_t, b, p.Lt);
    const int qi = blockIdx.x * 64 + (threadIdx.x >> 2), part = threadIdx.x & 3;
    const int qr = qi < Nq ? qi : Nq - 1;                       // rows past the end compute a copy and do not store
    float qs[DPL], qt[DPL], o[DPL];
    {
        const T* a = Qs + ((size_t)bh * Nq + qr) * DH + part * DPL;
        const T* c = Qt + ((size_t)bh * Nq + qr) * DH + part * DPL;
#pragma unroll
        for (int i = 0; i < DPL; ++i) { qs[i] = to_f32<T>(a[i]); qt[i] = to_f32<T>(c[i]); o[i] = 0.f; }
    }
    const T* ksb = Ks + (size_t)bh * p.Lsp * DH + part * DPL;
    const T* ktb = Kt + (size_t)bh * p.Ltp * DH + part * DPL;
    const T* vp = Vt + ((size_t)bh * DH + part * DPL) * p.Ltp;
    float ms = -INFINITY, ls = 0.f, mt = -INFINITY, lt = 0.f;   // pass 1
    for (int k = 0; k < ns; ++k) prob_online<EXP2>(ms, ls, quad_score<T, DPL>(ksb, k, qs));
    for (int j = 0; j < nt; ++j) prob_online<EXP2>(mt, lt, quad_score<T, DPL>(ktb, j, qt));
    const float is = 1.f / ls, it = 1.f / lt;

    for (int j = 0; j < nt; ++j) {
        const PairKey k = pair_key(p.ctl, p.Lt, b, j, ns);                  // (workgroup-uniform: the quads stay whole)
        const float pt = prob_exp<EXP2>(quad_score<T, DPL>(ktb, j, qt) - mt) * it;
        float ps = 0.f;
        if (k.has) ps = prob_exp<EXP2>(quad_score<T, DPL>(ksb, k.row, qs) - ms) * is;
        const float pj = pair_mix(k, pt, ps);
#pragma unroll
        for (int i = 0; i < DPL; ++i) o[i] = fmaf(pj, to_f32<T>(vp[(size_t)i * p.Ltp + j]), o[i]);
    }
    if (qi < Nq) {
        T* op = reinterpret_cast<T*>(p.out) + ((size_t)b * Nq + qi) * p.ldo + h * DH + part * DPL;
#pragma unroll
        for (int i = 0; i < DPL; ++i) op[i] = from_f32<T>(o[i]);
    }
}

template <typename T>
int control_valu(int dh, const void* Qs, const void* Ks, const void* Qt, const void* Kt, const void* Vt, const CtlParams& p, int B,
                 int use_exp2, hipStream_t s) {
    return pm_dh_dispatch("attention_control", dh, [&](auto dpl) {
        constexpr int DPL = decltype(dpl)::value;
        auto k = use_exp2 ? attention_control_valu_kernel<T, DPL, true> : attention_control_valu_kernel<T, DPL, false>;
        hipLaunchKernelGGL(k, dim3((p.Nq + 63) / 64, B * p.heads), dim3(256), 0, s, (const T*)Qs, (const T*)Ks, (const T*)Qt, (const T*)Kt,
                           (const T*)Vt, p);
    });
}

}  // namespace

extern "C" int pmhip_attention_control(int dtype, const void* Qs, const void* Ks, const void* Qt, const void* Kt, const void* Vt, void* out,
                                       int ldo, int B, int heads, int dim_head, int Nq, int Ls, int Ls_pad, int Lt, int Lt_pad,
                                       int use_exp2, const int32_t* row_map, const float* blend, const float* gain, const int32_t* lens_s,
                                       const int32_t* lens_t, pmhip_stream stream) {
    PM_TRY(pm_probs_check("attention_control", dtype, dim_head, heads, {{"Ls", Ls, Ls_pad}, {"Lt", Lt, Lt_pad}}));
    PM_REQUIRE(Qs && Ks && Qt && Kt && Vt && out, "attention_control: null pointer");
    PM_REQUIRE(row_map && blend && gain, "attention_control: row_map / blend / gain is NULL (pmhip_attention_lens is the entry without control)");
    PM_REQUIRE(B > 0 && heads > 0 && Nq > 0 && Ls > 0 && Lt > 0, "attention_control: empty problem");
    PM_REQUIRE(ldo >= heads * dim_head, "attention_control: ldo=%d is smaller than heads*dim_head=%d (rows of out would overlap)", ldo, heads * dim_head);
    PM_REQUIRE((long long)B * heads <= 65535, "attention_control: B*heads=%lld exceeds the grid's y range", (long long)B * heads);
    hipStream_t s = (hipStream_t)stream;
    CtlParams p{};
    p.out = out; p.ldo = ldo; p.heads = heads; p.Nq = Nq; p.Ls = Ls; p.Lsp = Ls_pad; p.Lt = Lt; p.Ltp = Lt_pad;
    p.ctl = {row_map, blend, gain}; p.lens_s = lens_s; p.lens_t = lens_t;
    const bool mfma = dtype == PMHIP_BF16 && dim_head == 64;
    if (mfma) {
        PM_REQUIRE(pm_aligned(16, {Qs, Ks, Qt, Kt}), "attention_control: Q and K must be 16-byte aligned");
        PM_REQUIRE(pm_aligned(8, {Vt, out}), "attention_control: Vt and out must be 8-byte aligned");
        PM_REQUIRE(Lt_pad % 4 == 0, "attention_control: Lt_pad=%d must be a multiple of 4 (8-byte V^T loads)", Lt_pad);
        PM_REQUIRE(ldo % 4 == 0, "attention_control: ldo=%d must be a multiple of 4 (8-byte row stores)", ldo);
    }
    PmTimer tm(FAM_ATTENTION, s);
    if (mfma) {
        auto k = use_exp2 ? attention_control_mfma_kernel<true> : attention_control_mfma_kernel<false>;
        hipLaunchKernelGGL(k, dim3((Nq + 63) / 64, B * heads), dim3(256), 0, s, (const bf16_t*)Qs, (const bf16_t*)Ks, (const bf16_t*)Qt,
                           (const bf16_t*)Kt, (const bf16_t*)Vt, p);
    } else if (dtype == PMHIP_F32) {
        PM_TRY(control_valu<float>(dim_head, Qs, Ks, Qt, Kt, Vt, p, B, use_exp2, s));
    } else {
        PM_TRY(control_valu<bf16_t>(dim_head, Qs, Ks, Qt, Kt, Vt, p, B, use_exp2, s));
    }
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}
