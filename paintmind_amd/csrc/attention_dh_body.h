// The plain-path attention kernel of attention_dh.hip (DPL = dims per lane = dh / 4), included once per form by attention_forms.h (no
// include guard on purpose; the forms, their flags and their trailing parameters are described there).  Particular to this kernel:
//   PM_ATTN_SEG   a key whose segment the query does not attend to (or padding, 255) is skipped -- its score and its V column are
//                 read by no update
//   PM_ATTN_BIAS  an allowed key's score becomes s + key_bias[b, k] before it meets the running maximum, and a key whose bias is
//                 -inf is skipped like padding
template <typename T, int DPL, bool EXP2>
__global__ __launch_bounds__(256) void PM_ATTN_KERNEL(const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ Vt,
                                                          T* __restrict__ out, int ldo, int heads, int Nq, int Nkv, int Nkp
#ifdef PM_ATTN_LENS
                                                            , const int* __restrict__ lens
#endif
#ifdef PM_ATTN_SEG
                                                            , const unsigned char* __restrict__ key_seg, const unsigned* __restrict__ query_mask
#endif
#ifdef PM_ATTN_BIAS
                                                            , const float* __restrict__ key_bias
#endif
#ifdef PM_ATTN_PICK
                                                            , const unsigned char* __restrict__ pick, int want
#endif
                                                            ) {
    constexpr int DH = DPL * 4;
    const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
#ifdef PM_ATTN_PICK
    // the picked form: a workgroup whose image is not the launch's kind is done here, before any load of the image's
    // rows and any store (workgroup-uniform: b is, and the flag goes through a scalar)
    if (__builtin_amdgcn_readfirstlane((int)pick[b]) != want) return;
#endif
#ifdef PM_ATTN_LENS
    {                                                           // workgroup-uniform: this image's key count
        const int n = __builtin_amdgcn_readfirstlane(lens[b]);
        Nkv = n < 1 ? 1 : (n > Nkv ? Nkv : n);
    }
#endif
    const int qi = blockIdx.x * 64 + (threadIdx.x >> 2), part = threadIdx.x & 3;
    const int qr = qi < Nq ? qi : Nq - 1;                       // rows past the end compute a copy and do not store
    float q[DPL], o[DPL];
    const T* qp = Q + ((size_t)bh * Nq + qr) * DH + part * DPL;
#pragma unroll
    for (int i = 0; i < DPL; ++i) { q[i] = to_f32<T>(qp[i]); o[i] = 0.f; }
    const T* kp = K + (size_t)bh * Nkp * DH + part * DPL;
    const T* vp = Vt + ((size_t)bh * DH + part * DPL) * Nkp;
    float m = -INFINITY, l = 0.f;
#ifdef PM_ATTN_SEG
    const unsigned char* segb = key_seg + (size_t)b * Nkv;
    const unsigned qm = query_mask[(size_t)b * Nq + qr];
#endif
#ifdef PM_ATTN_BIAS
    const float* biasb = key_bias + (size_t)b * Nkv;
#endif
    for (int j = 0; j < Nkv; ++j) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < DPL; ++i) s = fmaf(q[i], to_f32<T>(kp[(size_t)j * DH + i]), s);
        s = quad_sum(s);
#ifdef PM_ATTN_SEG
        const unsigned sg = segb[j];                            // (the four lanes of a query agree: the quad stays whole)
        if (!((sg < 32u) & ((qm >> (sg & 31u)) & 1u))) continue;
#endif
#ifdef PM_ATTN_BIAS
        const float kb = biasb[j];                              // (wave-uniform address: the quad stays whole here too)
        if (kb == -INFINITY) continue;
        s += kb;
#endif
        const float mn = fmaxf(m, s);
        const float a = EXP2 ? exp2f(m - mn) : expf(m - mn);
        const float pj = EXP2 ? exp2f(s - mn) : expf(s - mn);
        l = fmaf(l, a, pj);
#pragma unroll
        for (int i = 0; i < DPL; ++i) o[i] = fmaf(o[i], a, pj * to_f32<T>(vp[(size_t)i * Nkp + j]));
        m = mn;
    }
    if (qi < Nq) {
#ifdef PM_ATTN_SEG
        const float inv = l > 0.f ? 1.f / l : 0.f;              // (a query with no allowed key: a finite row)
#else
        const float inv = 1.f / l;
#endif
        T* op = out + ((size_t)b * Nq + qi) * ldo + h * DH + part * DPL;
#pragma unroll
        for (int i = 0; i < DPL; ++i) op[i] = from_f32<T>(o[i] * inv);
    }
}
