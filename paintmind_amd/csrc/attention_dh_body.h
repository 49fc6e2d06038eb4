// The plain-path attention kernel of attention_dh.hip (DPL = dims per lane = dh / 4), which includes this file TWICE (no include
// guard on purpose), exactly as attention_bf16.hip includes attention_bf16_body.h -- see there: PM_ATTN_KERNEL names the kernel,
// PM_ATTN_LENS_PARAM is empty or ", const int* lens", and with PM_ATTN_LENS the loop bound is lens[b], clamped to [1, Nkv].
template <typename T, int DPL, bool EXP2>
__global__ __launch_bounds__(256) void PM_ATTN_KERNEL(const T* __restrict__ Q, const T* __restrict__ K, const T* __restrict__ Vt,
                                                          T* __restrict__ out, int ldo, int heads, int Nq, int Nkv, int Nkp PM_ATTN_LENS_PARAM) {
    constexpr int DH = DPL * 4;
    const int bh = blockIdx.y, b = bh / heads, h = bh % heads;
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
    for (int j = 0; j < Nkv; ++j) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < DPL; ++i) s = fmaf(q[i], to_f32<T>(kp[(size_t)j * DH + i]), s);
        s = quad_sum(s);
        const float mn = fmaxf(m, s);
        const float a = EXP2 ? exp2f(m - mn) : expf(m - mn);
        const float pj = EXP2 ? exp2f(s - mn) : expf(s - mn);
        l = fmaf(l, a, pj);
#pragma unroll
        for (int i = 0; i < DPL; ++i) o[i] = fmaf(o[i], a, pj * to_f32<T>(vp[(size_t)i * Nkp + j]));
        m = mn;
    }
    if (qi < Nq) {
        const float inv = 1.f / l;
        T* op = out + ((size_t)b * Nq + qi) * ldo + h * DH + part * DPL;
#pragma unroll
        for (int i = 0; i < DPL; ++i) op[i] = from_f32<T>(o[i] * inv);
    }
}
