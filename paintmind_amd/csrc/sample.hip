// MaskGIT sampling tail (reference generate.py:163-179 with helpers :29-46), HBM-bound.
//
// sample_rows: ONE read of each logits row (32 KiB for 8192 fp32 classes).  One wave owns a row,
// the row lives in registers (16 B per lane per load, 1 KiB per wave-instruction, fully
// coalesced).  From that single residency the wave derives: the softmax normaliser (max, sum exp),
// the top-k candidates (k rounds of a wave-wide lexicographic arg-max -- no sort, no scatter of a
// -inf tensor as the reference does at :33-37), the gumbel-perturbed arg-max among the k candidates
// (noise is only needed at those k positions: every other position is -inf in the reference), the
// confidence of the unfiltered softmax at the sampled id, and the merge into the masked positions.
//
// sample_wide (top-k above 64, up to V: DESIGN.md section 4n): the same wave, row and normaliser; the kept set comes from a bitwise
// selection of the k-th value over the resident row instead of k rounds, and every lane draws among its own kept elements.
//
// sample_nucleus (top_p < 1, any top-k: DESIGN.md section 4o): the wide form's selection, then the kept elements' softmax weights
// in place of the keys and a bitwise search for the weight at which the mass from the top reaches top_p of the kept mass.
//
// sample_tiles (round 5, top-k <= 8 and V a multiple of 64: every launch of the decode loop): the same step from the softmax
// statistics of the row's 64-column blocks -- (max, sum of exp) per block, 8 bytes, left behind by the logits GEMM's epilogue
// (gemm_common.h, GemmParams::block_stats) -- and the k blocks with the largest maxima, which contain the k largest elements:
// 1 KiB + k x 256 B per row instead of 32 KiB.  Without statistics the kernel derives them from the stored row by the SAME
// arithmetic (common.h softmax_block_stat), so which kernel produced them never shows in the result.
//
// remask: per image, the num_mask highest scores get the mask id (generate.py:175-179); bitonic sort
// of 64-bit (score, reversed index) keys (remask_key) gives the exact (score desc, index asc) order; the keys stay in registers
// (remask_select, round 5; the all-LDS sort of rounds 1-4 is gone).  ONE kernel, remask_kernel<E, SLOTS, COUNTS, CHOICE>: the forms
// differ in where an image's count and choice values come from (image_step) and in whether the keys are perturbed (remask_choice_keys).
//
// The sampling kernels differ in how they find the k candidates and (the tiles kernel) in how they round the confidence.  Everything
// else is ONE piece of device code, each a function with its own signature: a wave's entry (wave_row, row_entry: the lane, the class
// test, the logits row) and where the row's step values come from (row_step: the kernel arguments, the PmGenParams block of a
// replayed graph, or the pmhip_slot record of the row's image -- common.h PmStepSource), the resident row and its normaliser
// (resident_row), an element's noise and perturbed value (perturbed), the draw among up to 64 candidates (draw_among) and the store
// of the row's outcome (store_outcome).  The host side has one launcher per kernel family (pm_sample_rows, pm_remask): one copy of
// the checks, one place that picks the instantiation.
// The one exception: the wide and the nucleus kernel still share their selection and their draw as two statement fragments,
// sample_select_prologue.h and sample_select_draw.h (each says what it expects in scope).  As functions they compute the same, but
// the register allocation of the 8192 and 16384 classes moves across an occupancy step (DESIGN.md section 4zj has the figures).
//
// Which of the four sampling kernels serves a row is pm_sample_class (common.h), a function of (top-k, top_p < 1).  A batch-scalar
// launch asks it once; a per-image launch with filters is four launches, one per class, in which every
// kernel's SLOTS form asks it per slot and serves the rows of its own class only (slot_in_class).
#include <stdlib.h>
#include <cmath>
#include <type_traits>

#include "common.h"

namespace {

constexpr int THREADS = 256;

struct Cand { float v; int i; };

// total order used everywhere: larger value first, then smaller index
__device__ __forceinline__ bool before(float av, int ai, float bv, int bi) {
    return (av > bv) || (av == bv && ai < bi);
}

// a float as an unsigned word of the same order (NaN aside): the keys of the re-masking sort and of the wide top-k's selection
__device__ __forceinline__ uint32_t orderable(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// wave-wide arg-max under `before`: a butterfly on the VALU only (DPP inside a row of 16 lanes, then the row / half swaps;
// nothing goes through the LDS pipe -- DESIGN.md section 4a).  Every lane ends with the same winner: the order is total.
__device__ __forceinline__ Cand wave_best(Cand c) {
    const int lane = threadIdx.x & 63;
#define PM_STEP(OV, OI) { const float ov = (OV); const int oi = (OI); if (before(ov, oi, c.v, c.i)) { c.v = ov; c.i = oi; } }
    PM_STEP(dpp_mov<0xB1>(c.v), dpp_mov<0xB1>(c.i))            // lane ^ 1
    PM_STEP(dpp_mov<0x4E>(c.v), dpp_mov<0x4E>(c.i))            // lane ^ 2
    PM_STEP(dpp_mov<0x141>(c.v), dpp_mov<0x141>(c.i))          // the other quad of the half row (quads are uniform now)
    PM_STEP(dpp_mov<0x140>(c.v), dpp_mov<0x140>(c.i))          // the other half row
    PM_STEP(__uint_as_float(other16(__float_as_uint(c.v), lane)), (int)other16((unsigned)c.i, lane))
    PM_STEP(__uint_as_float(other32(__float_as_uint(c.v), lane)), (int)other32((unsigned)c.i, lane))
#undef PM_STEP
    return c;
}

// wave-wide integer sum, the butterfly of wave_sum (common.h) on counts: every lane ends with the total
__device__ __forceinline__ int wave_count(int v) {
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    v += dpp_mov<0x140>(v);
    auto a = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    v = (int)(a[0] + a[1]);
    auto b = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    return (int)(b[0] + b[1]);
}

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

// log(t.clamp(min=1e-20)) twice, negated (generate.py:29-30,40-42)
__device__ __forceinline__ float gumbel_from_uniform(float u) {
    const float inner = -logf(fmaxf(u, 1e-20f));
    return -logf(fmaxf(inner, 1e-20f));
}

// ---- a row's step values.  Exactly one source (common.h PmStepSource): the kernel arguments as they are; gp != nullptr (graph
// replay): temperature, seed and row base from the device block, the step indexing it; SLOTS: everything from slots[row / tokens]
// -- one wave owns a row, so the values are wave-uniform like the kernel arguments they replace.  SLOTS is a compile-time choice:
// the scalar instantiations gain neither a load nor a branch.  `v` brings the kernel arguments; idle: the slot holds no request.
struct RowStep { int topk; float temperature; uint64_t seed; uint32_t step; uint64_t row_base; bool idle; };

template <bool SLOTS>
__device__ __forceinline__ RowStep row_step(RowStep v, int row, const PmGenParams* __restrict__ gp, const pmhip_slot* __restrict__ slots,
                                            int tokens) {
    if constexpr (SLOTS) {
        const int img = __builtin_amdgcn_readfirstlane(row / tokens);
        const pmhip_slot sl = slots[img];
        v.step = __builtin_amdgcn_readfirstlane(sl.step);
        v.idle = (v.step & PM_SLOT_IDLE) != 0;
        v.topk = __builtin_amdgcn_readfirstlane(sl.topk);
        v.temperature = sl.temperature;
        v.seed = sl.seed;
        // row_base + row = image_index * tokens + position (modulo 2^64, like the sum itself)
        v.row_base = sl.image_index * (uint64_t)tokens - (uint64_t)img * (uint64_t)tokens;
    } else if (gp) {
        v.temperature = gp->temps[v.step];
        v.seed = gp->seed;
        v.row_base = gp->row_base;
    }
    return v;
}

// ---- the class test of a per-image launch with filters (PmStepSource::with_filters).  The launcher issues
// one launch per class of pm_sample_class, and every row belongs to exactly one of them: the wave of a row whose slot is of another
// class returns before it touches any output, and so does the wave of an idle slot's row -- except in the block-statistics launch
// (class T), which writes the idle rows.  The slot's nucleus mass comes back in `top_p`: top_p_dev[image] (NULL: 1), wave-uniform
// like the record's values.  Only instantiated forms with SLOTS call this: the scalar forms gain nothing.
__device__ __forceinline__ bool slot_in_class(int cls, const RowStep& rs, int row, int tokens, const float* __restrict__ top_p_dev,
                                              float& top_p) {
    top_p = 1.f;
    if (top_p_dev) top_p = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(top_p_dev[row / tokens])));
    return !rs.idle && pm_sample_class(rs.topk, top_p < 1.f) == cls;
}

// ---- the entry of a sampling kernel: one wave per row.  wave_row() is the row; a wave whose row is >= M leaves at once, all its
// lanes together -- a test the kernel makes itself, in front of everything (a helper that made it, and handed the rest back through
// a flag, left the compiler a merged path on which a row's step values are resolved and held before the row is known to exist).
// row_entry then leaves the lane, the row's step values (row_step; `args` brings the kernel arguments), its nucleus mass (`top_p` as
// given, or the slot's), its logits row -- row % period under PERIOD -- and `served`: false only in a per-image launch with filters
// (CLS >= 0), for a live slot's row of another class.  The whole wave gets the same answer.  An idle slot's row comes back served
// with rs.idle set: the kernel decides (the block-statistics kernel writes it, the others leave).
__device__ __forceinline__ int wave_row() { return blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6); }

struct RowEntry { int lane; RowStep rs; float top_p; int lr; const float* lrow; bool served; };

template <bool SLOTS, bool PERIOD, int CLS = -1>
__device__ __forceinline__ RowEntry row_entry(int row, RowStep args, float top_p, const float* logits, int ldl, const PmGenParams* gp,
                                              int period, const pmhip_slot* slots, int tokens, const float* top_p_dev) {
    RowEntry en;
    en.lane = threadIdx.x & 63;
    en.rs = row_step<SLOTS>(args, row, gp, slots, tokens);
    en.top_p = top_p;
    en.served = true;
    if constexpr (SLOTS && CLS >= 0) en.served = slot_in_class(CLS, en.rs, row, tokens, top_p_dev, en.top_p) || en.rs.idle;
    en.lr = PERIOD ? row % period : row;
    en.lrow = logits + (size_t)en.lr * ldl;
    return en;
}

// ---- the step values of one image for the re-masking kernel (one workgroup per image): how many positions it masks and, for the
// CHOICE form, the choice temperature t and the image's Philox stream -- element i draws at counter
// (base + i, 0xFFFFFFFF, step) under the seed.  `v` brings the kernel arguments.  false: the workgroup leaves its row untouched.
// Every rule about the count is here and nowhere else:
//   the arguments / gp / the slot record as the source      num_mask, gp->nmask[step] or the record's, clamped to [1, N]; an idle
//                                                           slot leaves
//   COUNTS beside BATCH or PARAMS    c = counts[img]: c <= 0 leaves, c > N is the whole row
//   COUNTS beside SLOTS              an idle slot leaves whatever its count; c == 0 leaves; c < 0 is the
//                                                           record's num_mask with the clamp to 1; c > 0 is exactly c (above N: the row)
// The choice values never depend on COUNTS.  BATCH: the arguments, base = row_base + img * N; PARAMS: t = gp->ctemps[step], seed and
// row base from the block; SLOTS: t = choice[img] (a device float [B] beside the records), seed, step and image_index * N from the
// record, which is read once.
struct ImageStep { int num_mask; float t; uint64_t seed; uint32_t step; uint64_t base; };

template <bool SLOTS, bool COUNTS, bool CHOICE>
__device__ __forceinline__ bool image_step(ImageStep& v, int img, int N, const PmGenParams* gp, const pmhip_slot* slots,
                                           const int32_t* counts, const float* choice) {
    int c = -1;                                            // the table's count; below 0: the source's own
    if constexpr (COUNTS) {
        c = counts[img];
        if (SLOTS ? c == 0 : c <= 0) return false;
    }
    if constexpr (SLOTS) {
        const pmhip_slot sl = slots[img];
        if (sl.step & PM_SLOT_IDLE) return false;
        v.num_mask = sl.num_mask;
        if constexpr (CHOICE) {
            v.t = choice[img];
            v.seed = sl.seed;
            v.step = sl.step;
            v.base = sl.image_index * (uint64_t)N;
        }
    } else {
        if (gp) {
            v.num_mask = gp->nmask[v.step];
            if constexpr (CHOICE) {
                v.t = gp->ctemps[v.step];
                v.seed = gp->seed;
                v.base = gp->row_base;
            }
        }
        v.base += (uint64_t)img * (uint64_t)N;
    }
    if (c > 0) v.num_mask = c;
    v.num_mask = v.num_mask < 1 ? 1 : (v.num_mask > N ? N : v.num_mask);
    return true;
}

// ---- the perturbed value of one kept element (raw logit v at column col < V): v / max(T, 1e-10) + gumbel(u), u = noise[row][col]
// when noise is given, else Philox at (global row, column, step) under the seed, word .x, its top 24 bits.  u is a function of
// (row, column) and the step's values alone: which elements are kept, and how many, never moves the noise of one of them.
__device__ __forceinline__ float perturbed(float v, int col, int row, int V, const RowStep& st, const float* __restrict__ noise) {
    float u;
    if (noise) {
        u = noise[(size_t)row * V + col];
    } else {
        const uint64_t grow = st.row_base + (uint64_t)row;
        const uint4 rnd = philox4x32_10(make_uint4((uint32_t)grow, (uint32_t)(grow >> 32), (uint32_t)col, st.step),
                                        make_uint2((uint32_t)st.seed, (uint32_t)(st.seed >> 32)));
        u = (float)(rnd.x >> 8) * (1.0f / 16777216.0f);
    }
    return v / fmaxf(st.temperature, 1e-10f) + gumbel_from_uniform(u);
}

// ---- the draw: gumbel arg-max among the k candidates (lane r brings candidate r in `mine`: raw logit and column).  Noise is only
// needed at the candidates: given, or Philox at (global row, column, step) under the seed.  Every lane returns the sampled column
// and its RAW logit.
__device__ __forceinline__ Cand draw_among(Cand mine, int lane, int row, int V, const RowStep& st, const float* __restrict__ noise) {
    Cand pert{-INFINITY, 0x7fffffff};
    if (lane < st.topk && mine.i < V) {
        pert.v = perturbed(mine.v, mine.i, row, V, st, noise);
        pert.i = mine.i;
    }
    const Cand win = wave_best(pert);
    const unsigned long long owner = __ballot(lane < st.topk && mine.i == win.i);
    const int src = owner ? __ffsll((long long)owner) - 1 : 0;
    return Cand{__uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(mine.v), src)), win.i};   // src is wave-uniform
}

// ---- the store of a row's outcome, by one lane: the prediction, the id merged into the masked positions, and the score -- 1 - p
// where the position took the prediction, -1e5 where its id was given.  drawn = false (an idle slot): the row keeps its id.
__device__ __forceinline__ void store_outcome(int row, bool drawn, int64_t pred, float p, const int64_t* ids_in, int64_t mask_id,
                                              int64_t* pred_out, int64_t* ids_out, float* score_out) {
    const int64_t cur = ids_in[row];
    const bool take = drawn && cur == mask_id;
    if (pred_out) pred_out[row] = drawn ? pred : cur;
    ids_out[row] = take ? pred : cur;
    if (score_out) score_out[row] = take ? (1.0f - p) : -1e5f;
}

// Row layout in registers: lane l holds float4 group g (g = 0..NV4-1) = columns (g*64 + l)*4 .. +3,
// so a lane's columns increase with g and groups are disjoint contiguous column ranges: ordering
// candidates by (value desc, first column of their group asc) equals (value desc, column asc).
// PERIOD: logits row r is read from row r % period (every image of a batch samples from ONE image's logits -- the shared step 0 of
// an unconditional loop, engine.hip); ids, predictions, scores, the noise and the Philox counters stay per row.  The other
// instantiation never looks at `period`.
// SLOTS (a launch of class R for pmhip_sample_rows_slots_filter; no PERIOD form): the step values of row r come from slots[r /
// tokens] (row_step), and only the rows whose slot is of this kernel's class are served (slot_in_class); everything below the
// entry is the code of the scalar form.
// resident_row: the row into registers (a column >= V reads as -inf) and the softmax normaliser of the UNfiltered row
// (generate.py:170): max, sum of exp in lane order.  One copy of the expressions: the row, wide, nucleus and forced kernels give a
// drawn id the same confidence bits because they all come through here.
template <int NV4>
__device__ __forceinline__ void resident_row(float4 (&x)[NV4], float& mx, float& se, const float* lrow, int lane, int V) {
#pragma unroll
    for (int g = 0; g < NV4; ++g) {
        const int col = (g * 64 + lane) * 4;
        x[g] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        if (col < V) x[g] = *reinterpret_cast<const float4*>(lrow + col);
    }
    mx = -INFINITY;
#pragma unroll
    for (int g = 0; g < NV4; ++g) mx = fmaxf(mx, fmaxf(fmaxf(x[g].x, x[g].y), fmaxf(x[g].z, x[g].w)));
    mx = wave_max(mx);
    se = 0.f;
#pragma unroll
    for (int g = 0; g < NV4; ++g)
        se += (__expf(x[g].x - mx) + __expf(x[g].y - mx)) + (__expf(x[g].z - mx) + __expf(x[g].w - mx));
    se = wave_sum(se);
}

template <int NV4, bool PERIOD = false, bool SLOTS = false>
__global__ __launch_bounds__(THREADS) void sample_rows_kernel(
    const float* __restrict__ logits, int ldl, const int64_t* __restrict__ ids_in, int64_t mask_id, int topk,
    float temperature, const float* __restrict__ noise, uint64_t seed, uint32_t step, uint64_t row_base,
    int64_t* __restrict__ pred_out, int64_t* __restrict__ ids_out, float* __restrict__ score_out, int M, int V,
    const PmGenParams* __restrict__ gp, int period, const pmhip_slot* __restrict__ slots, int tokens,
    const float* __restrict__ top_p_dev) {
    const int row = wave_row();
    if (row >= M) return;                                  // whole wave exits together
    const RowEntry en = row_entry<SLOTS, PERIOD, PM_CLASS_ROWS>(row, RowStep{topk, temperature, seed, step, row_base, false}, 1.f, logits, ldl,
                                                                gp, period, slots, tokens, top_p_dev);
    if (!en.served || en.rs.idle) return;                  // (a per-image launch: the live rows of this class only)
    const int lane = en.lane;
    const RowStep& rs = en.rs;
    topk = rs.topk;                                        // (a slot's: wave-uniform, like the kernel argument it replaces)
    float4 x[NV4];
    float mx, se;
    resident_row<NV4>(x, mx, se, en.lrow, lane, V);

    // ---- top-k: k rounds of {per-lane best group, wave arg-max, winner removes its element}
    Cand mine{-INFINITY, 0x7fffffff};                      // candidate r is kept by lane r
#pragma unroll 1
    for (int r = 0; r < topk; ++r) {
        float bv = -INFINITY;
        int bg = 0;
#pragma unroll
        for (int g = 0; g < NV4; ++g) {
            const float m4 = fmaxf(fmaxf(x[g].x, x[g].y), fmaxf(x[g].z, x[g].w));
            if (m4 > bv) { bv = m4; bg = g; }              // strict: the first (lowest-column) group wins ties
        }
        Cand c{bv, (bg * 64 + lane) * 4};
        c = wave_best(c);
        // the owner lane finds the element inside the winning group and retires it
        const int wg = __builtin_amdgcn_readfirstlane(c.i >> 8);          // c.i = (g*64+lane)*4 -> g = c.i / 256
        const int wl = (c.i >> 2) & 63;
        int col = c.i;
#pragma unroll
        for (int g = 0; g < NV4; ++g) {
            if (g == wg) {                                                // wave-uniform branch
                if (lane == wl) {
                    if (x[g].x == c.v) { x[g].x = -INFINITY; col = c.i; }
                    else if (x[g].y == c.v) { x[g].y = -INFINITY; col = c.i + 1; }
                    else if (x[g].z == c.v) { x[g].z = -INFINITY; col = c.i + 2; }
                    else { x[g].w = -INFINITY; col = c.i + 3; }
                }
            }
        }
        col = __builtin_amdgcn_readlane(col, wl);                         // wl is wave-uniform
        if (lane == r) { mine.v = c.v; mine.i = col; }
    }
    // ---- the draw, and the confidence of the UNfiltered softmax at the sampled id.  The confidence is each kernel's own: here expf
    // and a plain division, over a denominator summed in lane order; in sample_tiles_kernel explicitly rounded operations over a
    // denominator summed block by block, so that the blocks' statistics can come from whoever computed them.  The two differ in
    // the last bits of the score, which is why the choice of the kernel depends on (V, top-k) only.
    const Cand win = draw_among(mine, lane, row, V, rs, noise);
    if (lane == 0) store_outcome(row, true, win.i, expf(win.v - mx) / se, ids_in, mask_id, pred_out, ids_out, score_out);
}

// ---- the wide form: 64 < top-k <= V.  Same wave, same resident row, same normaliser -- expression for
// expression, so the confidence of a drawn id has the bits sample_rows_kernel gives it -- but the kept set is found by selection
// instead of k rounds of arg-max, and every lane draws among its own kept elements instead of lane r among candidate r:
//   1. the row's values become their orderable() keys in place (-0 counts as +0, like `before`; a column >= V gets key 0, below
//      every value's);
//   2. tau = the k-th largest key, one bit per round from the top: a per-lane count of keys >= the trial value, one wave_count;
//   3. with g keys above tau, the k - g lowest COLUMNS among the keys equal to tau are kept: when there are more such keys than
//      that, the same search over the column bits finds the last kept column c (otherwise all of them are kept);
//   4. kept = key > tau, or key == tau and column <= c: exactly the first k elements of (value desc, column asc), one bit per
//      element in the lane's mask words.  top-k == V skips 2 and 3 (wave-uniform): tau = 0 and c = V - 1 keep every column < V;
//   5. each lane walks its mask from the lowest column up, reads the element's raw logit back (the row is in the cache it was just
//      loaded through), perturbs it (perturbed: the noise of a (row, column) does not depend on k) and keeps its best under
//      `before`; one wave_best finishes the draw, and the winner's lane hands over the raw logit.
// The walk is a loop of as many turns as the fullest lane has kept elements -- about k / 64 when the kept set is spread over
// the lanes -- with ONE copy of the Philox and the logarithms; the rounds of 2 and 3 are counted, never data-dependent.
// SLOTS: as in sample_rows_kernel -- a launch of class W.
template <int NV4, bool PERIOD = false, bool SLOTS = false>
__global__ __launch_bounds__(THREADS) void sample_wide_kernel(
    const float* __restrict__ logits, int ldl, const int64_t* __restrict__ ids_in, int64_t mask_id, int topk,
    float temperature, const float* __restrict__ noise, uint64_t seed, uint32_t step, uint64_t row_base,
    int64_t* __restrict__ pred_out, int64_t* __restrict__ ids_out, float* __restrict__ score_out, int M, int V,
    const PmGenParams* __restrict__ gp, int period, const pmhip_slot* __restrict__ slots, int tokens,
    const float* __restrict__ top_p_dev) {
    constexpr int CLS = PM_CLASS_WIDE;
    float top_p;                                           // (the class test's: this kernel has no use for the mass itself)
#include "sample_select_prologue.h"
    // ---- 4. the kept set, one bit per element: bit s = g * 4 + e of the lane's words, so a lane's columns rise with s
    constexpr int NW = (NV4 * 4 + 31) / 32;
    uint32_t kept[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) kept[w] = 0u;
    const int mine_last = last - lane * 4;
#pragma unroll
    for (int g = 0; g < NV4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int s = g * 4 + e;
            const bool keep = key[g][e] > tau || (key[g][e] == tau && g * 256 + e <= mine_last);   // last < V: no column beyond
            kept[s >> 5] |= (keep ? 1u : 0u) << (s & 31);
        }
#include "sample_select_draw.h"
}

// ---- the nucleus form: top_p < 1, every top-k in 1..V.  The wide kernel's wave, row, normaliser, top-k
// selection and draw; between the selection and the draw the kept set K shrinks to its nucleus:
//   a. every resident key becomes the element's weight w = __expf(x - max) for an element of K, 0 outside it and beyond V, held
//      as the bit pattern of a non-negative float -- whose unsigned order is the float order;
//   b. G(t) = the sum of the weights whose pattern is >= t: per lane in the fixed order of (g, e), then one wave_sum.  A sum of
//      non-negative terms, rounded to nearest in a fixed order, does not grow when terms are replaced by 0: G never increases in t,
//      as computed.  Z = G(1) (every positive weight) and P = top_p * Z, so G(1) >= P;
//   c. t* = the largest t with G(t) >= P, one bit per round over the 31 value bits -- counted rounds, never data-dependent;
//   d. kept = pattern >= t*: an element is kept iff the mass strictly above its weight, G(the next pattern), is below P; a
//      plateau of equal weights is kept or dropped whole, the row's maximum (mass 0 above it) always stays, a weight that
//      underflowed to 0 never does (t* >= 1).
// The filter reads the raw logits; the temperature acts in the draw only and the confidence stays the unfiltered softmax's.
// SLOTS: as in sample_rows_kernel -- a launch of class N; top_p is the slot's, top_p_dev[image].
template <int NV4, bool PERIOD = false, bool SLOTS = false>
__global__ __launch_bounds__(THREADS) void sample_nucleus_kernel(
    const float* __restrict__ logits, int ldl, const int64_t* __restrict__ ids_in, int64_t mask_id, int topk, float top_p,
    float temperature, const float* __restrict__ noise, uint64_t seed, uint32_t step, uint64_t row_base,
    int64_t* __restrict__ pred_out, int64_t* __restrict__ ids_out, float* __restrict__ score_out, int M, int V,
    const PmGenParams* __restrict__ gp, int period, const pmhip_slot* __restrict__ slots, int tokens,
    const float* __restrict__ top_p_dev) {
    constexpr int CLS = PM_CLASS_NUCLEUS;
#include "sample_select_prologue.h"
    // ---- a. weights in place of the keys (the value back from its key: orderable() undone)
    const int mine_last = last - lane * 4;
    uint32_t wt[NV4][4];
#pragma unroll
    for (int g = 0; g < NV4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t k = key[g][e];
            const float v = __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
            const bool in_k = k > tau || (k == tau && g * 256 + e <= mine_last);             // last < V: no column beyond
            wt[g][e] = in_k ? __float_as_uint(__expf(v - mx)) : 0u;
        }
    // ---- b., c. the mass threshold
    auto mass_from = [&](uint32_t t) -> float {
        float m = 0.f;
#pragma unroll
        for (int g = 0; g < NV4; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) m += wt[g][e] >= t ? __uint_as_float(wt[g][e]) : 0.f;
        return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(wave_sum(m))));
    };
    const float P = top_p * mass_from(1u);
    uint32_t ts = 0u;
#pragma unroll 1
    for (uint32_t bit = 0x40000000u; bit; bit >>= 1) {
        const uint32_t trial = ts | bit;
        if (mass_from(trial) >= P) ts = trial;
    }
    ts = max(ts, 1u);                                      // (a row whose sums are NaN finds nothing: still no zero weight, no column >= V)
    // ---- d. the kept set, one bit per element
    constexpr int NW = (NV4 * 4 + 31) / 32;
    uint32_t kept[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q) kept[q] = 0u;
#pragma unroll
    for (int g = 0; g < NV4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int s = g * 4 + e;
            kept[s >> 5] |= (wt[g][e] >= ts ? 1u : 0u) << (s & 31);
        }
#include "sample_select_draw.h"
}

// ---- the forced form (pmhip_sample_rows_forced): nothing is drawn -- the row's "prediction" is a GIVEN id,
// target[row], and the kernel scores it as the draw would have scored it.  Same wave, same resident row, same normaliser as
// sample_rows_kernel -- expression for expression, so for a target that a draw of the row, wide or nucleus kernel produced, the
// stored triple has that draw's bits.  Behind the normaliser: one load of the target's logit, by the lane that stores, and
// store_outcome with expf(v - mx) / se.  No top-k, no noise, no step values: no slots / params / period form.
// A target outside [0, V) is never used as an index: the range test sits in front of the load, and the row is stored as an undrawn
// row is (pred = merged = ids_in, score = -1e5).  The targets are device memory: the host cannot check them without a sync.
template <int NV4>
__global__ __launch_bounds__(THREADS) void sample_forced_kernel(
    const float* __restrict__ logits, int ldl, const int64_t* __restrict__ ids_in, const int64_t* __restrict__ target, int64_t mask_id,
    int64_t* __restrict__ pred_out, int64_t* __restrict__ ids_out, float* __restrict__ score_out, int M, int V) {
    const int row = wave_row();
    if (row >= M) return;                                  // whole wave exits together
    const RowEntry en = row_entry<false, false>(row, RowStep{}, 1.f, logits, ldl, nullptr, 0, nullptr, 0, nullptr);   // (no step values here)
    float4 x[NV4];
    float mx, se;
    resident_row<NV4>(x, mx, se, en.lrow, en.lane, V);

    if (en.lane == 0) {
        const int64_t t = target[row];
        const bool ok = t >= 0 && t < (int64_t)V;          // in front of the load: an id from outside indexes nothing
        float v = -INFINITY;
        if (ok) v = en.lrow[t];
        store_outcome(row, ok, t, expf(v - mx) / se, ids_in, mask_id, pred_out, ids_out, score_out);
    }
}


// ---- the step from block statistics -----------------------------------------------------------------------------------------
// (KT_MAX = 8, the top-k this kernel serves, and K_LANES sit beside pm_sample_class in common.h)
// NB2 = blocks per lane (block b is kept by lane b % 64).  DENSE: no statistics were handed in -- one pass over the stored row
// computes them (lane l, group g: columns (g*64 + l)*4 .. +3, i.e. block g*4 + l/16 in the layout softmax_block_stat defines).
// SLOTS (pmhip_sample_rows_slots): the step values of row r come from slots[r / tokens] (row_step); everything below the prologue
// is the code of the scalar form.
// PERIOD: as in sample_rows_kernel -- the logits AND the statistics of row r are those of row r % period.
// FILTER (with SLOTS; pmhip_sample_rows_slots_filter): the launch of class T beside those of the row kernels -- it writes the idle
// rows, as the SLOTS form does, and of the others those whose slot is of class T (slot_in_class).
template <int NB2, bool DENSE, bool SLOTS = false, bool PERIOD = false, bool FILTER = false>
__global__ __launch_bounds__(THREADS) void sample_tiles_kernel(
    const float* __restrict__ logits, int ldl, const float2* __restrict__ stats, const int64_t* __restrict__ ids_in, int64_t mask_id,
    int topk, float temperature, const float* __restrict__ noise, uint64_t seed, uint32_t step, uint64_t row_base,
    int64_t* __restrict__ pred_out, int64_t* __restrict__ ids_out, float* __restrict__ score_out, int M, int V,
    const PmGenParams* __restrict__ gp, const pmhip_slot* __restrict__ slots, int tokens, int period,
    const float* __restrict__ top_p_dev) {
    __shared__ float2 sh[DENSE ? THREADS / 64 : 1][DENSE ? NB2 * 64 : 1];
    const int row = wave_row(), wave = threadIdx.x >> 6;
    if (row >= M) return;                                  // whole wave exits together (no workgroup barrier below)
    const RowEntry en = row_entry<SLOTS, PERIOD, FILTER ? (int)PM_CLASS_TILES : -1>(row, RowStep{topk, temperature, seed, step, row_base, false},
                                                                                    1.f, logits, ldl, gp, period, slots, tokens, top_p_dev);
    const int lane = en.lane, lr = en.lr;
    const RowStep& rs = en.rs;
    if (!en.served) return;                                // (FILTER: a live slot's row of another class)
    if (SLOTS && rs.idle) {                                // wave-uniform: nothing is drawn, the row keeps its id
        if (lane == 0) store_outcome(row, false, 0, 0.f, ids_in, mask_id, pred_out, ids_out, score_out);
        return;
    }
    topk = rs.topk;
    const float* lrow = en.lrow;
    const int nblk = V >> 6;

    float2 st[NB2];
    if constexpr (DENSE) {
        const int ngroups = (V + 255) >> 8;
        for (int g0 = 0; g0 < ngroups; g0 += 8) {          // eight 1-KiB loads in flight per wave
            float4 x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int col = ((g0 + u) * 64 + lane) * 4;
                x[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (g0 + u < ngroups && col < V) x[u] = *reinterpret_cast<const float4*>(lrow + col);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int col = ((g0 + u) * 64 + lane) * 4;
                const float2 b = softmax_block_stat(x[u].x, x[u].y, x[u].z, x[u].w);
                if (g0 + u < ngroups && col < V && (lane & 15) == 0) sh[wave][(g0 + u) * 4 + (lane >> 4)] = b;
            }
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int j = 0; j < NB2; ++j) {
            const int b = lane + 64 * j;
            st[j] = b < nblk ? sh[wave][b] : make_float2(-INFINITY, 0.f);
        }
    } else {
        const float2* srow = stats + (size_t)lr * nblk;
#pragma unroll
        for (int j = 0; j < NB2; ++j) {
            const int b = lane + 64 * j;
            st[j] = b < nblk ? srow[b] : make_float2(-INFINITY, 0.f);
        }
    }
    // ---- softmax normaliser of the UNfiltered row (generate.py:170) from the blocks: max M, S = sum_b s_b 2^((m_b - M) log2 e)
    float mx = st[0].x;
#pragma unroll
    for (int j = 1; j < NB2; ++j) mx = fmaxf(mx, st[j].x);
    mx = wave_max(mx);
    float se = 0.f;
#pragma unroll
    for (int j = 0; j < NB2; ++j) se = __fmaf_rn(st[j].y, softmax_exp_below(st[j].x, mx), se);
    se = wave_sum(se);

    // ---- the k blocks with the largest maxima, (max desc, block asc): they hold the k first elements of (value desc, column asc)
    // (an element outside them has k blocks in front of its own, each with an element that comes before it)
    int tile[KT_MAX];
    float x[KT_MAX];
#pragma unroll
    for (int r = 0; r < KT_MAX; ++r) {
        tile[r] = -1;
        x[r] = -INFINITY;
        if (r < topk) {                                    // wave-uniform
            float bv = -INFINITY;
            int bj = 0;
#pragma unroll
            for (int j = 0; j < NB2; ++j)
                if (st[j].x > bv) { bv = st[j].x; bj = j; }   // strict: the lowest block wins ties
            Cand c{bv, lane + 64 * bj};
            c = wave_best(c);
            if (c.v > -INFINITY) {                         // (fewer blocks than k: the remaining rounds find nothing)
                tile[r] = __builtin_amdgcn_readfirstlane(c.i);
#pragma unroll
                for (int j = 0; j < NB2; ++j)
                    if (lane + 64 * j == c.i) st[j].x = -INFINITY;
                x[r] = lrow[tile[r] * 64 + lane];
            }
        }
    }
    // ---- top-k elements of the k x 64 values: k rounds of {per-lane best, wave arg-max, winner retires its element}
    Cand mine{-INFINITY, 0x7fffffff};                      // candidate r is kept by lane r
#pragma unroll
    for (int r = 0; r < KT_MAX; ++r) {
        if (r < topk) {
            Cand c{-INFINITY, 0x7fffffff};
#pragma unroll
            for (int q = 0; q < KT_MAX; ++q) {
                const int ci = tile[q] * 64 + lane;
                if (tile[q] >= 0 && before(x[q], ci, c.v, c.i)) { c.v = x[q]; c.i = ci; }
            }
            c = wave_best(c);
#pragma unroll
            for (int q = 0; q < KT_MAX; ++q)
                if (tile[q] >= 0 && tile[q] * 64 + lane == c.i) x[q] = -INFINITY;
            if (lane == r) mine = c;
        }
    }
    // ---- the draw, and the confidence (this kernel's own rounding: see sample_rows_kernel).  raw <= mx and se >= 1 (the
    // maximum's own term): p in [0, 1]
    const Cand win = draw_among(mine, lane, row, V, rs, noise);
    if (lane == 0)
        store_outcome(row, true, win.i, __fdiv_rn(softmax_exp_below(win.v, mx), se), ids_in, mask_id, pred_out, ids_out, score_out);
}

// the sort key: (score desc, index asc) as one descending 64-bit order
__device__ __forceinline__ unsigned long long remask_key(float score, int i) {
    return ((unsigned long long)orderable(score) << 32) | (unsigned long long)(0xffffffffu - (uint32_t)i);
}

// ---- the keys of the CHOICE form: MaskGIT's perturbed confidence.  With the image's choice temperature t
// (image_step) an element with score s sorts by
//   s                                                           t == 0 (the plain key, bit for bit), or s < 0 (a given id: no draw)
//   -fmaf(t, gumbel(u), logf(fmaxf(1 - s, 2^-24)))              otherwise
// u: noise_row[i] (given uniforms, the image's row: BATCH sources only), or Philox at (st.base + i, 0xFFFFFFFF, step) -- a column
// word no class column has (V <= 16384), so the stream never meets the token draw's.  t <= 1000 keeps every noisy key above the
// -1e5 of a given id; t is uniform over the workgroup.
template <int E>
__device__ __forceinline__ void remask_choice_keys(unsigned long long (&key)[E], unsigned long long* xs, const float* sc,
                                                   const float* noise_row, int base, int N, const ImageStep& st) {
    // one element at a time (a Philox and three logf each: unrolled E = 16 times they would not fit the registers), through the
    // thread's own E words of xs, which nobody else touches before the first barrier
#pragma unroll 1
    for (int e = 0; e < E; ++e) {
        const int i = base + e;
        unsigned long long k = 0ull;
        if (i < N) {
            float s = sc[i];
            if (st.t != 0.f && !(s < 0.f)) {
                float u;
                if (noise_row) {
                    u = noise_row[i];
                } else {
                    const uint64_t grow = st.base + (uint64_t)i;
                    const uint4 rnd = philox4x32_10(make_uint4((uint32_t)grow, (uint32_t)(grow >> 32), 0xFFFFFFFFu, st.step),
                                                    make_uint2((uint32_t)st.seed, (uint32_t)(st.seed >> 32)));
                    u = (float)(rnd.x >> 8) * (1.0f / 16777216.0f);
                }
                const float ph = 1.0f - s;
                const float conf = logf(fmaxf(ph, 0x1p-24f));
                s = -fmaf(st.t, gumbel_from_uniform(u), conf);
            }
            k = remask_key(s, i);
        }
        xs[i] = k;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) key[e] = xs[base + e];
}

// ---- the selection with the sort in registers (round 5).  Thread t keeps the E consecutive elements base = t*E .. t*E+E-1 in
// key[E] (sorted in place); mine[E] is a copy that stays.  A bitonic compare-exchange with distance j is in-thread for j < E, a
// wave shuffle for j < 64*E and goes through LDS (xs[THREADS * E], two barriers) only beyond that: 3 of the 55 stages at N = 1024
// (the all-LDS sort of rounds 1-4 had one barrier per stage, 40 us per launch on B <= 64 workgroups -- latency, not work).  Then the
// threshold, the num_mask-th key (num_mask in [1, N]: image_step), and the store of mask_id into the image's ids row.
template <int E>
__device__ __forceinline__ void remask_select(unsigned long long (&key)[E], const unsigned long long (&mine)[E], unsigned long long* xs,
                                              int base, int num_mask, int N, int64_t* ids_row, int64_t mask_id) {
    constexpr int NP = THREADS * E;
#pragma unroll
    for (int k = 2; k <= NP; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            if (j < E) {                                   // both elements in this thread
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    if ((e & j) == 0) {
                        const bool desc = ((base + e) & k) == 0;
                        const unsigned long long a = key[e], b = key[e | j];
                        const bool swap = desc ? (a < b) : (a > b);
                        key[e] = swap ? b : a;
                        key[e | j] = swap ? a : b;
                    }
                }
            } else {
                unsigned long long other[E];
                if (j < 64 * E) {                          // the partner thread is in this wave
#pragma unroll
                    for (int e = 0; e < E; ++e) other[e] = __shfl_xor(key[e], j / E, 64);
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e) xs[base + e] = key[e];
                    __syncthreads();
#pragma unroll
                    for (int e = 0; e < E; ++e) other[e] = xs[(base + e) ^ j];
                    __syncthreads();
                }
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int i = base + e;
                    const bool want_max = ((i & j) == 0) == ((i & k) == 0);   // descending block: the lower index keeps the larger key
                    const unsigned long long a = key[e], b = other[e];
                    key[e] = want_max ? (a > b ? a : b) : (a < b ? a : b);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) xs[base + e] = key[e];
    __syncthreads();
    const unsigned long long thr = xs[num_mask - 1];
    const int inside = N - base;                           // base + e < N as e < inside: one register for the E tests, not E indices
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (e < inside && mine[e] >= thr) ids_row[base + e] = mask_id;
}

// ---- the re-masking kernel: one workgroup per image, every form of every entry (pmhip_remask*).  SLOTS, COUNTS and CHOICE say
// where the image's count and choice values come from -- image_step resolves them, and every early exit is there, before the
// first barrier; the forms differ in nothing else.  A form leaves the arguments it has no use for unread.
template <int E, bool SLOTS, bool COUNTS, bool CHOICE>
__global__ __launch_bounds__(THREADS) void remask_kernel(int64_t* __restrict__ ids, const float* __restrict__ scores, int num_mask,
                                                         int64_t mask_id, int N, const PmGenParams* __restrict__ gp, int step,
                                                         const pmhip_slot* __restrict__ slots, const int32_t* __restrict__ counts,
                                                         float choice_t, const float* __restrict__ choice,
                                                         const float* __restrict__ noise, uint64_t seed, uint64_t row_base) {
    __shared__ unsigned long long xs[THREADS * E];
    const int img = blockIdx.x;
    ImageStep st{num_mask, choice_t, seed, (uint32_t)step, row_base};
    if (!image_step<SLOTS, COUNTS, CHOICE>(st, img, N, gp, slots, counts, choice)) return;
    const int base = threadIdx.x * E;
    const float* sc = scores + (size_t)img * N;
    unsigned long long key[E], mine[E];
    if constexpr (CHOICE) {
        remask_choice_keys<E>(key, xs, sc, SLOTS || !noise ? nullptr : noise + (size_t)img * N, base, N, st);
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const int i = base + e;
            key[e] = i < N ? remask_key(sc[i], i) : 0ull;   // the plain key; an element beyond the row sorts below every real one
        }
    }
#pragma unroll
    for (int e = 0; e < E; ++e) mine[e] = key[e];
    remask_select<E>(key, mine, xs, base, st.num_mask, N, ids + (size_t)img * N, mask_id);
}

// a run-time size class or flag as a compile-time constant: f(std::integral_constant<int, V>) for the one V of Vs that equals v
template <int... Vs, typename F>
void pick(int v, F&& f) {
    ((v == Vs ? f(std::integral_constant<int, Vs>{}) : (void)0), ...);
}

// the size class of the kernels with a resident row: NV4, the float4 groups a lane holds, for a row of V <= 16384 classes
int nv4_class(int V) { return V <= 256 ? 1 : V <= 1024 ? 4 : V <= 8192 ? 32 : 64; }

}  // namespace

int pm_sample_rows(const float* logits, int ldl, const float* block_stats, int period, const int64_t* ids_in, int64_t mask_id,
                   const float* noise, int64_t* pred_out, int64_t* ids_out, float* score_out, int M, int V, const PmStepSource& src,
                   pmhip_stream stream) {
    const bool slots = src.kind == PmStepSource::SLOTS;
    const char* who = slots ? "sample_rows_slots" : "sample_rows";
    PM_REQUIRE(logits && ids_in && ids_out && (!slots || src.slots) && (src.kind != PmStepSource::PARAMS || src.gp), "%s: null pointer", who);
    PM_REQUIRE(period >= 0 && !(slots && period), "%s: bad logits row period %d", who, period);
    PM_TRY(pm_check_top_p(who, src.top_p));
    const bool nucleus = src.top_p < 1.f;
    PM_REQUIRE(!(slots && nucleus), "%s: top_p=%g: the per-image records carry no top_p (the nucleus filter is the batch forms')", who, (double)src.top_p);
    PM_REQUIRE(M > 0 && V > 0 && V % 4 == 0 && ldl % 4 == 0 && ldl >= V, "%s: bad shape M=%d V=%d ldl=%d", who, M, V, ldl);
    if (slots) {                                           // the block-statistics kernel only: what every decode-loop launch runs
        PM_REQUIRE(V % 64 == 0 && V <= 16384, "sample_rows_slots: V=%d must be a multiple of 64, at most 16384", V);
        PM_REQUIRE(src.tokens > 0 && M % src.tokens == 0, "sample_rows_slots: M=%d is not a whole number of images of %d tokens", M, src.tokens);
    } else {
        PM_REQUIRE(src.topk >= 1 && src.topk <= V, "sample_rows: topk=%d must be in [1, V=%d]", src.topk, V);
        PM_REQUIRE(V <= 16384, "sample_rows: V=%d > 16384 unsupported", V);
    }
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(ceil_div(M, THREADS / 64)), block(THREADS);
    PmTimer tm(FAM_SAMPLE, s);
    // Which kernel runs depends on (V, topk) ONLY -- never on whether statistics were handed in: the two differ in the last bits
    // of the confidence (sample_rows_kernel); above top-k = 8 statistics are ignored.  The records of a slots launch carry
    // top-k <= 8 (checked where they are staged) -- unless the source asks for the filters: then every class gets its launch.
    // top_p < 1: the nucleus kernel for EVERY top-k -- the choice is a function of (V, topk, top_p < 1),
    // pm_sample_class; a scalar launch of class T whose V is no multiple of 64 (or with the dev switch off) runs on the row kernel.
    static const int g_tiles = pm_dev_knob("PMHIP_SAMPLE_TILES", 1);     // 0: the one-read row kernel everywhere (A/B)
    const bool filters = slots && src.filters;
    // one launch of class `cls`; PER_IMAGE: the form that serves the rows of its class only (a filters source)
    auto launch = [&](int cls, auto PER_IMAGE) {
        constexpr bool PI = decltype(PER_IMAGE)::value == 1;
        const int nv4 = nv4_class(V);
        if (cls == PM_CLASS_NUCLEUS) {
            pick<1, 4, 32, 64>(nv4, [&](auto NV4) {
                pick<0, 1>(!PI && period != 0, [&](auto PER) {
                    if constexpr (!(PI && PER() == 1))
                        hipLaunchKernelGGL((sample_nucleus_kernel<NV4(), PER() == 1, PI>), grid, block, 0, s, logits, ldl, ids_in, mask_id,
                                           src.topk, src.top_p, src.temperature, noise, src.seed, src.step, src.row_base, pred_out, ids_out,
                                           score_out, M, V, src.gp, period, src.slots, src.tokens, src.top_p_dev);
                });
            });
        } else if (cls == PM_CLASS_TILES) {
            const float2* st = reinterpret_cast<const float2*>(block_stats);
            pick<1, 2, 4>(V <= 4096 ? 1 : V <= 8192 ? 2 : 4, [&](auto NB2) {
                pick<0, 1>(st == nullptr, [&](auto DENSE) {
                    // scalar, period, slots, or slots as one class among four: never two of them
                    pick<0, 1, 2, 3>(PI ? 3 : slots ? 2 : period ? 1 : 0, [&](auto FORM) {
                        if constexpr (PI == (FORM() == 3))
                            hipLaunchKernelGGL((sample_tiles_kernel<NB2(), DENSE() == 1, FORM() >= 2, FORM() == 1, FORM() == 3>), grid, block, 0, s,
                                               logits, ldl, st, ids_in, mask_id, src.topk, src.temperature, noise, src.seed, src.step, src.row_base,
                                               pred_out, ids_out, score_out, M, V, src.gp, src.slots, src.tokens, period, src.top_p_dev);
                    });
                });
            });
        } else {
            // the row kernels: candidate r in lane r up to top-k = 64 (K_LANES), the selection above it
            pick<1, 4, 32, 64>(nv4, [&](auto NV4) {
                pick<0, 1>(!PI && period != 0, [&](auto PER) {
                    pick<0, 1>(cls == PM_CLASS_WIDE, [&](auto WIDE) {
                        if constexpr (!(PI && PER() == 1)) {
                            auto kernel = WIDE() == 1 ? sample_wide_kernel<NV4(), PER() == 1, PI> : sample_rows_kernel<NV4(), PER() == 1, PI>;
                            hipLaunchKernelGGL(kernel, grid, block, 0, s, logits, ldl, ids_in, mask_id, src.topk, src.temperature, noise, src.seed,
                                               src.step, src.row_base, pred_out, ids_out, score_out, M, V, src.gp, period, src.slots, src.tokens,
                                               src.top_p_dev);
                        }
                    });
                });
            });
        }
    };
    if (filters) {
        // T, R, W, N in this order on the stream: every row is written by exactly one of them (slot_in_class), the idle rows by T
        for (int cls : {PM_CLASS_TILES, PM_CLASS_ROWS, PM_CLASS_WIDE, PM_CLASS_NUCLEUS}) launch(cls, std::integral_constant<int, 1>{});
    } else {
        int cls = slots ? (int)PM_CLASS_TILES : pm_sample_class(src.topk, nucleus);
        if (cls == PM_CLASS_TILES && !slots && !(g_tiles && V % 64 == 0)) cls = PM_CLASS_ROWS;
        launch(cls, std::integral_constant<int, 0>{});
    }
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

extern "C" int pmhip_sample_rows(const float* logits, int ldl, const int64_t* ids_in, int64_t mask_id, int topk,
                                 float temperature, const float* noise, uint64_t seed, uint32_t step,
                                 uint64_t row_base, int64_t* pred_out, int64_t* ids_out, float* score_out, int M,
                                 int V, pmhip_stream stream) {
    return pm_sample_rows(logits, ldl, nullptr, 0, ids_in, mask_id, noise, pred_out, ids_out, score_out, M, V,
                          PmStepSource::batch(topk, temperature, 0, seed, step, row_base), stream);
}

// the same step with a nucleus filter behind the top-k (top_p == 1: exactly pmhip_sample_rows)
extern "C" int pmhip_sample_rows_nucleus(const float* logits, int ldl, const int64_t* ids_in, int64_t mask_id, int topk, float top_p,
                                         float temperature, const float* noise, uint64_t seed, uint32_t step, uint64_t row_base,
                                         int64_t* pred_out, int64_t* ids_out, float* score_out, int M, int V, pmhip_stream stream) {
    return pm_sample_rows(logits, ldl, nullptr, 0, ids_in, mask_id, noise, pred_out, ids_out, score_out, M, V,
                          PmStepSource::batch(topk, temperature, 0, seed, step, row_base).with_top_p(top_p), stream);
}

// the same step with the block statistics pmhip_gemm_softmax_stats (or pmhip_guidance_combine_stats) left behind: [M][V/64][2]
extern "C" int pmhip_sample_rows_stats(const float* logits, int ldl, const float* block_stats, const int64_t* ids_in, int64_t mask_id,
                                       int topk, float temperature, const float* noise, uint64_t seed, uint32_t step,
                                       uint64_t row_base, int64_t* pred_out, int64_t* ids_out, float* score_out, int M, int V,
                                       pmhip_stream stream) {
    PM_REQUIRE(block_stats, "sample_rows_stats: null statistics");
    PM_REQUIRE(V % 64 == 0, "sample_rows_stats: V=%d must be a multiple of 64", V);
    return pm_sample_rows(logits, ldl, block_stats, 0, ids_in, mask_id, noise, pred_out, ids_out, score_out, M, V,
                          PmStepSource::batch(topk, temperature, 0, seed, step, row_base), stream);
}

// the per-image form: every step value from slots[row / tokens]
extern "C" int pmhip_sample_rows_slots(const float* logits, int ldl, const float* block_stats, const int64_t* ids_in, int64_t mask_id,
                                       const pmhip_slot* slots, int tokens, int64_t* pred_out, int64_t* ids_out, float* score_out,
                                       int M, int V, pmhip_stream stream) {
    return pm_sample_rows(logits, ldl, block_stats, 0, ids_in, mask_id, nullptr, pred_out, ids_out, score_out, M, V,
                          PmStepSource::per_image(slots, tokens), stream);
}

// ... with the sampler filters per image: top-k in 1..V from the record, the nucleus mass from top_p_dev [B] (NULL: every slot 1);
// one launch per class of pm_sample_class
extern "C" int pmhip_sample_rows_slots_filter(const float* logits, int ldl, const float* block_stats, const int64_t* ids_in, int64_t mask_id,
                                              const pmhip_slot* slots, const float* top_p_dev, int tokens, int64_t* pred_out,
                                              int64_t* ids_out, float* score_out, int M, int V, pmhip_stream stream) {
    return pm_sample_rows(logits, ldl, block_stats, 0, ids_in, mask_id, nullptr, pred_out, ids_out, score_out, M, V,
                          PmStepSource::per_image(slots, tokens).with_filters(top_p_dev), stream);
}

// the forced step: target[row] in place of a draw, scored by the unfiltered softmax as a draw scores its id
extern "C" int pmhip_sample_rows_forced(const float* logits, int ldl, const int64_t* ids_in, const int64_t* target, int64_t mask_id,
                                        int64_t* pred_out, int64_t* ids_out, float* score_out, int M, int V, pmhip_stream stream) {
    const char* who = "sample_rows_forced";
    PM_REQUIRE(logits, "%s: logits is NULL", who);
    PM_REQUIRE(ids_in, "%s: ids_in is NULL", who);
    PM_REQUIRE(target, "%s: target is NULL", who);
    PM_REQUIRE(ids_out, "%s: ids_out is NULL", who);
    PM_REQUIRE(M > 0, "%s: M=%d must be positive", who, M);
    PM_REQUIRE(V > 0 && V <= 16384 && V % 4 == 0, "%s: V=%d must be a positive multiple of 4, at most 16384", who, V);
    PM_REQUIRE(ldl % 4 == 0 && ldl >= V, "%s: ldl=%d must be a multiple of 4, at least V=%d", who, ldl, V);
    hipStream_t s = (hipStream_t)stream;
    dim3 grid(ceil_div(M, THREADS / 64)), block(THREADS);
    PmTimer tm(FAM_SAMPLE, s);
    pick<1, 4, 32, 64>(nv4_class(V), [&](auto NV4) {
        hipLaunchKernelGGL((sample_forced_kernel<NV4()>), grid, block, 0, s, logits, ldl, ids_in, target, mask_id, pred_out, ids_out, score_out,
                           M, V);
    });
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

int pm_check_top_p(const char* who, float p) {
    PM_REQUIRE(std::isfinite(p) && p > 0.f && p <= 1.f, "%s: top_p=%g must be finite and in (0, 1]", who, (double)p);
    return PMHIP_OK;
}

int pm_check_choice_t(const char* who, float t) {
    PM_REQUIRE(std::isfinite(t) && t >= 0.f && t <= PM_CHOICE_T_MAX, "%s: the choice temperature %g must be finite and in [0, %g]", who, (double)t,
               (double)PM_CHOICE_T_MAX);
    return PMHIP_OK;
}

int pm_remask(int64_t* ids, const float* scores, int64_t mask_id, int B, int N, const PmStepSource& src, pmhip_stream stream) {
    const bool slots = src.kind == PmStepSource::SLOTS;
    const bool counts = src.counts != nullptr;             // the count of image b from counts[b]; everything else from the source's kind
    const bool choice = src.choice_on();
    char who[32];                                          // the entry's name, as the forms spell it
    snprintf(who, sizeof who, "remask%s%s%s", choice ? "_choice" : "", slots ? "_slots" : "", counts ? "_counts" : "");
    PM_REQUIRE(ids && scores && (!slots || src.slots) && (src.kind != PmStepSource::PARAMS || src.gp), "%s: null pointer", who);
    PM_REQUIRE(B > 0 && N > 0 && N <= 4096, "%s: bad shape B=%d N=%d (N <= 4096)", who, B, N);
    int per_thread = 1;                                    // E: the power of two with THREADS * E >= N
    while (THREADS * per_thread < N) per_thread <<= 1;
    hipStream_t s = (hipStream_t)stream;
    PmTimer tm(FAM_SAMPLE, s);
    pick<1, 2, 4, 8, 16>(per_thread, [&](auto E) {
        pick<0, 1, 2, 3, 4, 5, 6, 7>((slots ? 4 : 0) | (counts ? 2 : 0) | (choice ? 1 : 0), [&](auto FORM) {
            hipLaunchKernelGGL((remask_kernel<E(), (FORM() & 4) != 0, (FORM() & 2) != 0, (FORM() & 1) != 0>), dim3(B), dim3(THREADS), 0, s, ids,
                               scores, src.num_mask, mask_id, N, src.gp, (int)src.step, src.slots, src.counts, src.choice_t, src.choice_dev,
                               src.choice_noise, src.seed, src.row_base);
        });
    });
    PM_HIP(hipGetLastError());
    return PMHIP_OK;
}

extern "C" int pmhip_remask(int64_t* ids, const float* scores, int num_mask, int64_t mask_id, int B, int N,
                            pmhip_stream stream) {
    return pm_remask(ids, scores, mask_id, B, N, PmStepSource::batch(0, 0.f, num_mask, 0, 0, 0), stream);
}

extern "C" int pmhip_remask_slots(int64_t* ids, const float* scores, const pmhip_slot* slots, int64_t mask_id, int B, int N,
                                  pmhip_stream stream) {
    return pm_remask(ids, scores, mask_id, B, N, PmStepSource::per_image(slots, N), stream);
}

// the choice forms: the checks that concern the choice arguments, then the one launcher (choice_t == 0 without given noise IS
// pmhip_remask: the plain kernel)
extern "C" int pmhip_remask_choice(int64_t* ids, const float* scores, int num_mask, int64_t mask_id, int B, int N, float choice_t,
                                   const float* noise, uint64_t seed, uint32_t step, uint64_t row_base, pmhip_stream stream) {
    PM_TRY(pm_check_choice_t("remask_choice", choice_t));
    return pm_remask(ids, scores, mask_id, B, N, PmStepSource::batch(0, 0.f, num_mask, seed, step, row_base).with_choice(choice_t, noise), stream);
}

extern "C" int pmhip_remask_choice_slots(int64_t* ids, const float* scores, const pmhip_slot* slots, const float* choice_t_dev,
                                         int64_t mask_id, int B, int N, pmhip_stream stream) {
    PM_REQUIRE(choice_t_dev, "remask_choice_slots: null pointer");
    return pm_remask(ids, scores, mask_id, B, N, PmStepSource::per_image(slots, N).with_choice_dev(choice_t_dev), stream);
}

// the slot forms with a count per slot: counts_dev[b] < 0 the record's num_mask (the entries above on that
// row), 0 the row untouched, > 0 exactly that many (the counts entries below on that row, with the slot's seed, step and image index)
extern "C" int pmhip_remask_slots_counts(int64_t* ids, const float* scores, const pmhip_slot* slots, const int32_t* counts_dev,
                                         int64_t mask_id, int B, int N, pmhip_stream stream) {
    PM_REQUIRE(slots && counts_dev, "remask_slots_counts: null pointer");
    return pm_remask(ids, scores, mask_id, B, N, PmStepSource::per_image(slots, N).with_counts(counts_dev), stream);
}

extern "C" int pmhip_remask_choice_slots_counts(int64_t* ids, const float* scores, const pmhip_slot* slots, const float* choice_t_dev,
                                                const int32_t* counts_dev, int64_t mask_id, int B, int N, pmhip_stream stream) {
    PM_REQUIRE(slots && choice_t_dev && counts_dev, "remask_choice_slots_counts: null pointer");
    return pm_remask(ids, scores, mask_id, B, N, PmStepSource::per_image(slots, N).with_choice_dev(choice_t_dev).with_counts(counts_dev), stream);
}

// the counts forms: image b re-masks counts_dev[b] positions, 0 leaving its row untouched; row b is
// pmhip_remask / pmhip_remask_choice on that row alone with num_mask = counts_dev[b] (noise at row_base + b * N), bit for bit
extern "C" int pmhip_remask_counts(int64_t* ids, const float* scores, const int32_t* counts_dev, int64_t mask_id, int B, int N,
                                   pmhip_stream stream) {
    PM_REQUIRE(counts_dev, "remask_counts: null pointer");
    return pm_remask(ids, scores, mask_id, B, N, PmStepSource::batch(0, 0.f, 0, 0, 0, 0).with_counts(counts_dev), stream);
}

extern "C" int pmhip_remask_choice_counts(int64_t* ids, const float* scores, const int32_t* counts_dev, int64_t mask_id, int B, int N,
                                          float choice_t, const float* noise, uint64_t seed, uint32_t step, uint64_t row_base,
                                          pmhip_stream stream) {
    PM_REQUIRE(counts_dev, "remask_choice_counts: null pointer");
    PM_TRY(pm_check_choice_t("remask_choice_counts", choice_t));
    return pm_remask(ids, scores, mask_id, B, N,
                     PmStepSource::batch(0, 0.f, 0, seed, step, row_base).with_choice(choice_t, noise).with_counts(counts_dev), stream);
}
