// Shared device/host helpers for libpaintmind_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <atomic>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pmhip.h"
#include "attention_forms.h"

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef unsigned short bf16_t;  // storage type of a bfloat16 element

// ---------------------------------------------------------------------------------------------
// error plumbing (never throws across the C ABI)
// ---------------------------------------------------------------------------------------------
void pm_set_error(const char* fmt, ...);

#define PM_HIP(expr)                                                                    \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            pm_set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return PMHIP_EHIP;                                                          \
        }                                                                               \
    } while (0)

#define PM_REQUIRE(cond, ...)                  \
    do {                                       \
        if (!(cond)) {                         \
            pm_set_error(__VA_ARGS__);         \
            return PMHIP_EINVAL;               \
        }                                      \
    } while (0)

#define PM_TRY(expr)                \
    do {                            \
        int _rc = (expr);           \
        if (_rc != PMHIP_OK) return _rc; \
    } while (0)

// ---------------------------------------------------------------------------------------------
// per-family kernel timing (bench.py's roofline leg).  Off by default: zero overhead.
// ---------------------------------------------------------------------------------------------
// The GEMM launches are kept per kind so that bench.py can price every kernel of the family against its own roofline:
//   FAM_GEMM        plain (bias only): logits, patch embedding, prev_quant, the decoder's pixel projection, context projection
//   FAM_GEMM_HEADS  head-split q|k|v projections          FAM_GEMM_SWIGLU  w12 with the gate in the epilogue
//   FAM_GEMM_RESID  residual producers on the 256x256 / 128x128 kernels (FFN w3, token / post-quant projections)
//   FAM_GEMM_RESID2B  residual producers on the two-workgroups-per-CU kernel (attention out-projections)
// pmhip_timing_get("gemm") is the sum of the five.
enum PmFamily { FAM_GEMM = 0, FAM_ATTENTION, FAM_LAYERNORM, FAM_SAMPLE, FAM_VQ, FAM_ROWOPS, FAM_GEMM_HEADS, FAM_GEMM_SWIGLU, FAM_GEMM_RESID,
                FAM_GEMM_RESID2B, FAM_COUNT };
struct PmTimer {
    PmTimer(int family, hipStream_t s);
    ~PmTimer();
    int family;
    hipStream_t stream;
    hipEvent_t e0;
    bool on;
};
extern std::atomic<bool> g_pm_timing_on;

// ---------------------------------------------------------------------------------------------
// per-call scalars of a hipGraph-replayed decode loop (device memory, refreshed before every replay)
// ---------------------------------------------------------------------------------------------
constexpr int PM_MAX_STEPS = 128;
struct PmGenParams {
    unsigned long long seed;
    unsigned long long row_base;
    float temps[PM_MAX_STEPS];
    int nmask[PM_MAX_STEPS];
    float ctemps[PM_MAX_STEPS];     // choice temperatures (the choice form of the re-masking kernel); appended: nothing above moves
    float gscales[PM_MAX_STEPS];    // guidance scales of a scheduled loop (pmhip_guidance_combine_dev reads &gscales[t]); appended
};
static_assert(offsetof(PmGenParams, ctemps) == 16 + 8 * PM_MAX_STEPS, "PmGenParams: the fields in front of ctemps keep their offsets");
static_assert(offsetof(PmGenParams, gscales) == 16 + 12 * PM_MAX_STEPS, "PmGenParams: the fields in front of gscales keep their offsets");

// ---------------------------------------------------------------------------------------------
// per-IMAGE decode state (include/pmhip.h, pmhip_slot): device memory, one record per image of the batch.  The slots forms of the
// sampling tail read every per-call value from it, so a captured step serves every schedule and every mix of requests.
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(pmhip_slot) == 32, "pmhip_slot is 32 bytes: two 16-byte words per image");
constexpr uint32_t PM_SLOT_IDLE = 0x80000000u;              // bit 31 of pmhip_slot::step

// ---------------------------------------------------------------------------------------------
// Where a launch of the sampling tail takes its step values from -- exactly one of
//   BATCH   the scalars below, one set for every row;
//   PARAMS  a replayed graph: temperature, mask count, seed and row base from the device block gp, indexed by `step`; top-k and
//           the step stay kernel arguments (they are part of the graph);
//   SLOTS   per image: the device records slots [M / tokens] (V % 64 == 0; the block-statistics kernel only, top-k <= 8 and no top_p --
//           unless with_filters() asks for the launch per class).
// ---------------------------------------------------------------------------------------------
struct PmStepSource {
    enum Kind { BATCH, PARAMS, SLOTS } kind;
    int topk; float temperature; int num_mask; uint64_t seed; uint32_t step; uint64_t row_base;
    const PmGenParams* gp;
    const pmhip_slot* slots; int tokens;
    static PmStepSource batch(int topk, float temperature, int num_mask, uint64_t seed, uint32_t step, uint64_t row_base) {
        return {BATCH, topk, temperature, num_mask, seed, step, row_base, nullptr, nullptr, 0};
    }
    static PmStepSource params(const PmGenParams* gp, int topk, uint32_t step) { return {PARAMS, topk, 0.f, 0, 0, step, 0, gp, nullptr, 0}; }
    static PmStepSource per_image(const pmhip_slot* slots, int tokens) { return {SLOTS, 0, 0.f, 0, 0, 0, 0, nullptr, slots, tokens}; }
    // The choice temperature of the re-masking step (pm_remask only), by the same three sources: BATCH the
    // scalar choice_t with optional given uniforms [B,N]; PARAMS gp->ctemps[step]; SLOTS the device array choice_dev [B].  Off
    // (the default): the plain re-masking kernel, as before.
    float choice_t = 0.f; const float* choice_noise = nullptr; const float* choice_dev = nullptr; bool choice_params = false;
    bool choice_on() const { return kind == BATCH ? (choice_t != 0.f || choice_noise) : kind == PARAMS ? choice_params : choice_dev != nullptr; }
    PmStepSource with_choice(float t, const float* noise) const { PmStepSource r = *this; r.choice_t = t; r.choice_noise = noise; return r; }
    PmStepSource with_choice_params() const { PmStepSource r = *this; r.choice_params = true; return r; }
    PmStepSource with_choice_dev(const float* dev) const { PmStepSource r = *this; r.choice_dev = dev; return r; }
    // The nucleus filter of the token draw (pm_sample_rows only): of the top-k elements, those whose mass
    // strictly above them is below top_p of the top-k's mass.  BATCH and PARAMS only -- a kernel argument, like top-k; a SLOTS
    // source with top_p < 1 is refused.  1 (the default): no filter, the kernels that ran before.
    float top_p = 1.f;
    PmStepSource with_top_p(float p) const { PmStepSource r = *this; r.top_p = p; return r; }
    // The re-masking count PER IMAGE (pm_remask only): a device int32 [B] beside a BATCH or PARAMS source --
    // image b re-masks counts[b] positions instead of num_mask / gp->nmask[step], 0 leaving its row untouched; the choice values keep
    // coming from the source's kind.  NULL (the default): the source's own count.
    // Beside a SLOTS source the table is a count per SLOT: counts[b] < 0 the record's num_mask (with its clamp
    // to 1), 0 the row untouched, > 0 exactly that many; the step values from the record.  Every form is an instantiation of the one
    // re-masking kernel (sample.hip remask_kernel<E, SLOTS, COUNTS, CHOICE>), and image_step there states each rule once.
    const int32_t* counts = nullptr;
    PmStepSource with_counts(const int32_t* dev) const { PmStepSource r = *this; r.counts = dev; return r; }
    // The sampler filters PER IMAGE (pm_sample_rows only, a SLOTS source): every slot's top-k in 1..V and its
    // nucleus mass from top_p_dev, a device float [B] beside the records (NULL: every slot 1) -- the launcher then issues one launch
    // per class of pm_sample_class, each serving the rows of its class.  Off (the default): the one block-statistics launch, top-k
    // <= 8, as before.  Appended: nothing above moves.
    const float* top_p_dev = nullptr; bool filters = false;
    PmStepSource with_filters(const float* dev) const { PmStepSource r = *this; r.top_p_dev = dev; r.filters = true; return r; }
};
// Which sampling kernel serves a row: a function of (top-k, top_p < 1) ONLY -- the kernels differ in the last bits of the
// confidence, so a request's rows run on the kernel its own scalar run picks, whatever shares the batch.
// The scalar launcher and the per-image kernels both ask here.  (A scalar launch whose V is no multiple of 64 serves class T on
// the row kernel: pm_sample_rows.)
constexpr int KT_MAX = 8;                                  // top-k served by sample_tiles_kernel
constexpr int K_LANES = 64;                                // top-k served by sample_rows_kernel: one candidate per lane
enum PmSampleClass { PM_CLASS_TILES = 0, PM_CLASS_ROWS = 1, PM_CLASS_WIDE = 2, PM_CLASS_NUCLEUS = 3 };
__host__ __device__ inline int pm_sample_class(int topk, bool nucleus) {
    return nucleus ? PM_CLASS_NUCLEUS : topk <= KT_MAX ? PM_CLASS_TILES : topk <= K_LANES ? PM_CLASS_ROWS : PM_CLASS_WIDE;
}
// a step's nucleus mass: finite, 0 < top_p <= 1
int pm_check_top_p(const char* who, float p);
// a step's choice temperature: finite, 0 <= t <= 1000 (the bound keeps every noisy key above the -1e5 of a given id)
constexpr float PM_CHOICE_T_MAX = 1000.f;
int pm_check_choice_t(const char* who, float t);
// block_stats: NULL, or the (max, sum of exp) pairs of the row's 64-column blocks, [M][V/64][2] (softmax_block_stat below)
// period: 0, or the number of logits (and statistics) rows there are -- row r then samples from row r % period
int pm_sample_rows(const float* logits, int ldl, const float* block_stats, int period, const int64_t* ids_in, int64_t mask_id,
                   const float* noise, int64_t* pred_out, int64_t* ids_out, float* score_out, int M, int V, const PmStepSource& src,
                   pmhip_stream stream);
int pm_remask(int64_t* ids, const float* scores, int64_t mask_id, int B, int N, const PmStepSource& src, pmhip_stream stream);

// ---------------------------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float bf16_to_f32(bf16_t h) { return __uint_as_float(((uint32_t)h) << 16); }

// fp32 -> bf16, round-to-nearest-even (what torch's float->bfloat16 cast does); the casts lower to
// the hardware v_cvt_pk_bf16_f32
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
__device__ __forceinline__ bf16_t f32_to_bf16(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    bf16x2_t v;
    v[0] = (__bf16)lo;
    v[1] = (__bf16)hi;
    return __builtin_bit_cast(uint32_t, v);
}

template <typename T> __device__ __forceinline__ T from_f32(float f);
template <> __device__ __forceinline__ float from_f32<float>(float f) { return f; }
template <> __device__ __forceinline__ bf16_t from_f32<bf16_t>(float f) { return f32_to_bf16(f); }

template <typename T> __device__ __forceinline__ float to_f32(T v);
template <> __device__ __forceinline__ float to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float to_f32<bf16_t>(bf16_t v) { return bf16_to_f32(v); }

// store 4 consecutive elements (p is 4-element aligned)
__device__ __forceinline__ void store4(float* p, float a, float b, float c, float d) {
    *reinterpret_cast<float4*>(p) = make_float4(a, b, c, d);
}
__device__ __forceinline__ void store4(bf16_t* p, float a, float b, float c, float d) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(a, b), pack_bf16x2(c, d));
}

// store 16 consecutive elements (p is 16-byte aligned)
__device__ __forceinline__ void store16(float* p, const float (&v)[16]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(p + 4 * j) = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
}
__device__ __forceinline__ void store16(bf16_t* p, const float (&v)[16]) {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    *reinterpret_cast<uint4*>(p + 8) = make_uint4(pack_bf16x2(v[8], v[9]), pack_bf16x2(v[10], v[11]), pack_bf16x2(v[12], v[13]), pack_bf16x2(v[14], v[15]));
}

// one 16-byte store: 4 floats or 8 bf16
__device__ __forceinline__ void store_row(float* p, const float (&v)[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store_row(bf16_t* p, const float (&v)[8]) {
    *reinterpret_cast<uint4*>(p) = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
}

// One 16-byte operand chunk per lane feeds the matrix core:
//   bf16: 8 k-values  -> one  v_mfma_f32_16x16x32_bf16
//   f32 : 4 k-values  -> four v_mfma_f32_16x16x4_f32 (exact f32, == an fmaf chain)
// `first` supplies the ROWS of the 16x16 result, `second` the COLUMNS; result element
// (row 4*(lane>>4)+r, col lane&15) lands in acc[r].  The k <-> (lane>>4, element) assignment is
// identical for both operands, so any consistent chunk layout contracts correctly.
template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
    static constexpr int kElemsPerChunk = 8;
    __device__ static __forceinline__ void run(f32x4_t& acc, const uint4& first, const uint4& second) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, first),
                                                      __builtin_bit_cast(bf16x8_t, second), acc, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    static constexpr int kElemsPerChunk = 4;
    __device__ static __forceinline__ void run(f32x4_t& acc, const uint4& first, const uint4& second) {
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(first.x), __uint_as_float(second.x), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(first.y), __uint_as_float(second.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(first.z), __uint_as_float(second.z), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(first.w), __uint_as_float(second.w), acc, 0, 0, 0);
    }
};

// async global -> LDS copy of 16 B per lane; LDS destination = wave-uniform base + lane*16
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// Wave-wide butterfly reductions on the VALU only (DPP within a row of 16 lanes, then the gfx950 row / half swaps):
// no ds_bpermute, so nothing goes through the LDS pipe and no lgkmcnt wait sits between the steps.
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v) {
    return __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(v), CTRL, 0xf, 0xf, true));
}
template <int CTRL> __device__ __forceinline__ int dpp_mov(int v) {
    return (int)__builtin_amdgcn_update_dpp(0u, (unsigned)v, CTRL, 0xf, 0xf, true);
}
// value held by the OTHER row pair member (lane ^ 16) / the other half (lane ^ 32): for symmetric butterflies
__device__ __forceinline__ unsigned other16(unsigned v, int lane) {
    auto a = __builtin_amdgcn_permlane16_swap(v, v, false, false);       // a[0] = {row0,row0,row2,row2}, a[1] = {row1,row1,row3,row3}
    return (lane & 16) ? a[0] : a[1];
}
__device__ __forceinline__ unsigned other32(unsigned v, int lane) {
    auto a = __builtin_amdgcn_permlane32_swap(v, v, false, false);       // a[0] = {lo,lo}, a[1] = {hi,hi}
    return (lane & 32) ? a[0] : a[1];
}
#ifdef PM_WAVE_REDUCE_BPERMUTE
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
#else
// quad_perm [1,0,3,2] = 0xB1 (lane^1), quad_perm [2,3,0,1] = 0x4E (lane^2), row_half_mirror = 0x141 (the other quad of
// the 8-lane half row once the quads are uniform), row_mirror = 0x140 (the other half row); then rows and halves
__device__ __forceinline__ float wave_sum(float v) {
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    v += dpp_mov<0x140>(v);
    {
        auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
        auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = __uint_as_float(b[0]) + __uint_as_float(b[1]);
    }
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    v = fmaxf(v, dpp_mov<0x140>(v));
    {
        auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1]));
        auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        v = fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
    }
    return v;
}
#endif

// max without the canonicalising `v_max x,x,x` hipcc puts in front of fmaxf() on MFMA results
__device__ __forceinline__ float vmax2(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// reductions over the 4 lanes {l, l^16, l^32, l^48} with the gfx950 row / half swaps (no LDS round trip):
// permlane16_swap(v,v) -> {rows 0,0,2,2 | rows 1,1,3,3}, permlane32_swap(v,v) -> {lo,lo | hi,hi}
__device__ __forceinline__ float group4_max(float v) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const float m = vmax2(__uint_as_float(a[0]), __uint_as_float(a[1]));
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    return vmax2(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float group4_sum(float v) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const float m = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
// sum over the 4 lanes of a quad {4 i .. 4 i + 3}: two DPP steps
__device__ __forceinline__ float quad_sum(float v) {
    v += dpp_mov<0xB1>(v);      // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);      // quad_perm [2,3,0,1]
    return v;
}

// ------------------------------------------------------------------------------------------------
// LayerNorm fold: per-row (rstd, -rstd * mean) from the partial statistics a hi/lo producer left behind (per 64-column part:
// sum, and sum of squares centred on the part's own mean).  ONE definition of the arithmetic -- explicitly rounded operations
// in a fixed tree -- shared by pmhip_ln_coef_parts' kernel (8 lanes per row, DPP sums) and by the folded small-batch GEMM that
// computes the coefficients of its own rows in its prologue (one lane per row): both produce the same bits, so whether the
// separate kernel runs may depend on the batch size although an image's result may not.
//   part j of a row is paired with part j + 8 (missing parts count as zero); the eight pair values are summed as
//   ((0+1)+(2+3)) + ((4+5)+(6+7))
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float lnp_m2_term(float2 part, float mean) {        // centred sum of squares of one part about the ROW mean
    const float d = __fsub_rn(__fmul_rn(part.x, 1.0f / 64.0f), mean);
    return __fmaf_rn(__fmul_rn(64.0f, d), d, part.y);
}
__device__ __forceinline__ float lnp_mean(float total, int nparts) { return __fdiv_rn(total, (float)(nparts * 64)); }
__device__ __forceinline__ float2 lnp_finish(float m2, float mean, int nparts, float eps) {
    const float rstd = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(__fdiv_rn(m2, (float)(nparts * 64)), eps)));
    return make_float2(rstd, __fmul_rn(-rstd, mean));
}
__device__ __forceinline__ float lnp_tree8(const float (&v)[8]) {
    return __fadd_rn(__fadd_rn(__fadd_rn(v[0], v[1]), __fadd_rn(v[2], v[3])), __fadd_rn(__fadd_rn(v[4], v[5]), __fadd_rn(v[6], v[7])));
}
// one lane, one row: pr = the row's nparts (sum, centred sum of squares) pairs, nparts <= 16.  Load and arithmetic are separate
// so that a caller can request the pairs early and combine them late.
__device__ __forceinline__ void ln_coef_row_load(const float2* pr, int nparts, float2 (&pa)[8], float2 (&pb)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        pa[j] = j < nparts ? pr[j] : make_float2(0.f, 0.f);
        pb[j] = j + 8 < nparts ? pr[j + 8] : make_float2(0.f, 0.f);
    }
}
__device__ __forceinline__ float2 ln_coef_row(const float2 (&pa)[8], const float2 (&pb)[8], int nparts, float eps) {
    float sv[8], mv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) sv[j] = __fadd_rn(pa[j].x, pb[j].x);
    const float mean = lnp_mean(lnp_tree8(sv), nparts);
#pragma unroll
    for (int j = 0; j < 8; ++j)
        mv[j] = __fadd_rn(j < nparts ? lnp_m2_term(pa[j], mean) : 0.f, j + 8 < nparts ? lnp_m2_term(pb[j], mean) : 0.f);
    return lnp_finish(lnp_tree8(mv), mean, nparts, eps);
}

// ------------------------------------------------------------------------------------------------
// Softmax statistics of one 64-column block of a logits row: (m, s) = (max, sum_j 2^((x_j - m) log2 e)).  ONE definition of
// the arithmetic -- explicitly rounded operations in a fixed tree -- shared by the f32 GEMM epilogue (gemm_common.h: the block is
// the 64 columns a wave owns, at the point where it stores them), the guidance combination (rowops.hip) and the sampling kernel
// when it has to derive them from a stored row (sample.hip): the same logits give the same bits whoever computes them, so a
// step's result does not depend on which kernel produced the statistics.
//   layout: the 16 lanes of a DPP row, lane j holding columns 4j .. 4j+3; every lane of the row returns the block's pair
// ------------------------------------------------------------------------------------------------
constexpr float PM_LOG2E = 1.4426950408889634f;
// e^(x - m) for x <= m.  The difference is taken FIRST: x = m gives exactly 1, and the rounding error of the exponent scales with
// |x - m|, not with |m|.  (fma(x, log2 e, -rn(m log2 e)) carries the rounding error of m log2 e, up to 2^-19 for |m| in 22..44: a
// row with one dominant class got p = 1 -+ 1.3e-6 instead of 1 and a confidence score below 0 or above it by that much.)
__device__ __forceinline__ float softmax_exp_below(float x, float m) {
    return __builtin_amdgcn_exp2f(__fmul_rn(__fsub_rn(x, m), PM_LOG2E));
}
__device__ __forceinline__ float2 softmax_block_stat(float a, float b, float c, float d) {
    float m = fmaxf(fmaxf(a, b), fmaxf(c, d));
    m = fmaxf(m, dpp_mov<0xB1>(m));
    m = fmaxf(m, dpp_mov<0x4E>(m));
    m = fmaxf(m, dpp_mov<0x141>(m));
    m = fmaxf(m, dpp_mov<0x140>(m));
    float s = __fadd_rn(__fadd_rn(softmax_exp_below(a, m), softmax_exp_below(b, m)), __fadd_rn(softmax_exp_below(c, m), softmax_exp_below(d, m)));
    s = __fadd_rn(s, dpp_mov<0xB1>(s));
    s = __fadd_rn(s, dpp_mov<0x4E>(s));
    s = __fadd_rn(s, dpp_mov<0x141>(s));
    s = __fadd_rn(s, dpp_mov<0x140>(s));
    return make_float2(m, s);
}

// DEVELOPMENT KNOBS: tuning values and the switches of finished A/Bs (tools/*.sh sweep them).  They are read from the environment
// only in a development build (PM_EXTRA_FLAGS=-DPM_DEV_KNOBS bash paintmind_amd/csrc/build.sh); the product library carries the
// defaults as constants -- no configuration that no test runs (round-5 review, W6).  The switches the tests DO exercise stay
// runtime: PMHIP_HILO, PMHIP_LN_UNFOLD, PMHIP_HILO_CENTER, PMHIP_FOLD_MAX_ROWS (engine.hip Switches).
static inline int pm_dev_knob(const char* name, int dflt) {
#ifdef PM_DEV_KNOBS
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
#else
    (void)name;
    return dflt;
#endif
}

static inline int ceil_div(int a, int b) { return (a + b - 1) / b; }
static inline size_t dtype_size(int dtype) { return dtype == PMHIP_BF16 ? 2 : 4; }

// One attention launch: operands, geometry, the optional arrays of the forms (attention_forms.h) and the stream.  The
// pointers that are set select the form -- pm_attn_form --, and pm_attn_check is the one place that says which may stand together.
struct PmAttnArgs {
    const void *Q, *K, *Vt;
    void* out;
    int ldo, B, heads, Nq, Nkv, Nkv_pad, use_exp2;
    const int* lens = nullptr;                   // device int32 [B], or NULL: one key count for the launch
    const unsigned char* key_seg = nullptr;      // device uint8 [B, Nkv] and ...
    const unsigned* query_mask = nullptr;        // ... device uint32 [B, Nq], or both NULL
    const float* key_bias = nullptr;             // device f32 [B, Nkv], or NULL
    const unsigned char* pick = nullptr;         // device uint8 [B], or NULL: the launch serves every image
    int want = 0;
    hipStream_t stream = nullptr;
};
inline PmAttnForm pm_attn_form(const PmAttnArgs& a) {
    if (a.key_seg) return a.key_bias ? (a.pick ? PM_FORM_SEG_BIAS_PICK : PM_FORM_SEG_BIAS) : (a.pick ? PM_FORM_SEG_PICK : PM_FORM_SEG);
    return a.lens ? (a.pick ? PM_FORM_LENS_PICK : PM_FORM_LENS) : PM_FORM_PLAIN;
}
// key_seg and query_mask go together; lens and that pair exclude each other; key_bias needs the pair; pick needs exactly one of lens
// and the pair, and want in [0, 255].  Looks at the optional arrays only (pmhip_attention_maps fills nothing else).
int pm_attn_check(const char* who, const PmAttnArgs& a);
// Every attention launch ends here (attention_dh.hip): the arguments are checked once, then one launcher per kernel file, each
// already past the checks.  who = the entry point's name in error texts.
int attention_any(const char* who, int dtype, int dim_head, const PmAttnArgs& a);
void pm_attention_f32(const PmAttnArgs& a);      // attention.hip: fp32, dim_head = 64
void pm_attention_bf16(const PmAttnArgs& a);     // attention_bf16.hip: bf16, dim_head = 64
// The vector-ALU attention kernels are templates over DPL = dim_head / 4, the dims a lane owns: THE list of the values served.
// f(std::integral_constant<int, DPL>) launches the caller's instantiation; any other dim_head is refused under the entry's name.
template <typename F>
int pm_dh_dispatch(const char* who, int dh, F&& f) {
    switch (dh / 4) {
#define PM_DH_CASE(n) case n: f(std::integral_constant<int, n>{}); break;
        PM_DH_CASE(4) PM_DH_CASE(8) PM_DH_CASE(12) PM_DH_CASE(16) PM_DH_CASE(20) PM_DH_CASE(24) PM_DH_CASE(28) PM_DH_CASE(32)
#undef PM_DH_CASE
        default: PM_REQUIRE(false, "%s: dim_head=%d not served", who, dh);
    }
    return PMHIP_OK;
}
// What the entries that recompute probabilities (attention_maps.hip, attention_control.hip, attention_phrase.hip) ask of every call:
// a dtype, dim_head a multiple of 16 in [16, 128], heads <= 64, and every context's padded length at least its length.
struct PmContext { const char* name; int len, pad; };
int pm_probs_check(const char* who, int dtype, int dim_head, int heads, std::initializer_list<PmContext> contexts);
// every pointer a multiple of `bytes` (the 16-byte fragment loads of the MFMA routes)
inline bool pm_aligned(size_t bytes, std::initializer_list<const void*> ptrs) {
    uintptr_t all = 0;
    for (const void* p : ptrs) all |= (uintptr_t)p;
    return all % bytes == 0;
}

// Can a LayerNorm over K columns be folded into the GEMM out[M,N] = A[M,K] (row stride lda) . W[N,K]^T (row stride ldw)?  THE
// predicate: the engine's decision (M = one image's rows: folded or not must not depend on the batch), the GEMM entry points'
// check and pmhip_lnfold_supported all ask it.  M, N whole 256x256 tiles, K whole pairs of K-tiles, and both operands within the
// 32-bit byte offsets the 256x256 kernel addresses them with.
inline bool pm_lnfold_shape_ok(int M, int N, int K, int lda, int ldw) {
    return M % 256 == 0 && N % 256 == 0 && K % 128 == 0 && K >= 128 && (unsigned long long)M * lda * 2 < (1ull << 31) &&
           (unsigned long long)N * ldw * 2 < (1ull << 31);
}
