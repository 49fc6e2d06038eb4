/*
 * pmhip.h -- C ABI of libpaintmind_hip.so: the MI355X (gfx950) generation path of PaintMind.
 *
 * The reference (Qiyuan-Ge/PaintMind) has no FFI: its boundary is a Python object protocol whose
 * arithmetic is delegated to PyTorch ATen.  This header is the boundary a maintainer would bind
 * instead (ctypes stub in INTEGRATION.md).  Every entry point cites the reference code whose
 * arithmetic it replaces (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain pointers + sizes only; all pointers are DEVICE pointers unless the name ends in _host
 *   - `stream` is a hipStream_t passed as void*; every call is asynchronous on that stream
 *   - return value: 0 = ok, otherwise a PMHIP_E* code; pmhip_last_error() gives the message
 *     (thread-local).  Nothing throws across this boundary.
 *   - the caller owns every tensor and every weight; the library owns only its handles'
 *     workspace arenas (hipMalloc'ed, grown on demand, freed by *_destroy)
 *   - handles are single-stream objects, not thread-safe
 *   - matrices are row-major; "T" below is the handle's compute dtype (PMHIP_F32 or PMHIP_BF16);
 *     weights are stored [out_features, in_features] exactly like torch.nn.Linear
 *   - GEMM reduction widths (K) must be multiples of 64 elements; the host packer zero-pads
 *
 * Memory contract (tests/test_gpu_abi_memory.py holds every operator to it)
 *   - leading dimensions (lda, ldw, ldr, ldo, ldl) count ELEMENTS between the starts of consecutive rows and may be wider than
 *     the row: the gap is never written and what it holds (NaN included) never reaches a result.  Lower bounds, checked
 *     (PMHIP_EINVAL, the message names the argument):
 *         lda >= K, ldw >= K          every GEMM entry point (and both multiples of 8)
 *         ldo >= N, ldr >= N          pmhip_gemm / _ln / _softmax_stats (ldr only with a residual), pmhip_gemm_hilo / _stats / _center
 *         ldo >= Hp                   pmhip_gemm_swiglu / _ln
 *         ldo >= heads * dim_head     pmhip_attention / _dh / _lens / _control
 *         ldm >= Nkv                  pmhip_attention_maps
 *         ldl >= V                    pmhip_sample_rows / _stats / _slots / _nucleus / _forced, pmhip_masked_ce, pmhip_logit_divergence,
 *                                     pmhip_token_logprob
 *     A result does not depend on a leading dimension: the same values give the same bits at any ld (as long as M * lda and
 *     N * ldw stay below 2^30 elements; beyond that another kernel may serve the call).
 *   - an output of [M, N] is written in exactly its M x N elements, however ragged M and N are against a kernel's tile; arrays
 *     without a leading dimension (row_stats, block_stats, coef, shift, pred, ids, score, ...) in exactly their stated extent
 *   - in place is allowed where an entry point says so, and only there:
 *         pmhip_gemm_hilo / _stats / _center   out_hi == res_hi and out_lo == res_lo with ldo == ldr, the residual being the
 *                                              stream itself (res_rows <= 0 or >= M: no row modulo)
 *         pmhip_gemm with an f32 residual      out == residual with ldo == ldr, res_rows covering all M rows
 *         pmhip_unshift_hilo, pmhip_remask(_slots), pmhip_remask_choice(_slots), pmhip_guidance_combine(_stats), pmhip_sample_rows* (ids_out == ids_in)
 *         pmhip_remask_counts, pmhip_remask_choice_counts, pmhip_mask_tokens (ids), pmhip_composite (out == gen or orig)
 *         pmhip_remask_slots_counts, pmhip_remask_choice_slots_counts
 *         pmhip_guidance_combine_slots(_which) out == cond (or uncond / other)
 *     Every element is read by the workgroup that writes it, before it writes it; the result equals the out-of-place call's bit
 *     for bit.  Any other overlap between an output and an input is undefined.
 */
#ifndef PMHIP_H
#define PMHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMHIP_ABI_VERSION 11

enum { PMHIP_OK = 0, PMHIP_EINVAL = 1, PMHIP_EHIP = 2, PMHIP_ENOMEM = 3, PMHIP_ESTATE = 4 };
enum { PMHIP_F32 = 0, PMHIP_BF16 = 1 };
/* what a block of packed projection rows is, for pmhip_gemm_heads */
enum { PMHIP_PART_Q = 0, PMHIP_PART_K = 1, PMHIP_PART_V = 2 };

typedef void* pmhip_stream;

int pmhip_abi_version(void);
const char* pmhip_last_error(void);
/* number of compute units / LDS bytes per workgroup / gcnArchName of `device` */
int pmhip_device_info(int device, int* cu_count, int* lds_bytes, char* arch, int arch_len);

/* ------------------------------------------------------------------------------------------------
 * Operator level (stateless).  These are what the reference's operator plug-point would call
 * (Layer.ATTENTION_MODES, stage1/layers.py:41-48, stage2/transformer.py:29-36; SwiGLU swap,
 * modules/mlp.py:34-40).
 * ---------------------------------------------------------------------------------------------- */

/* out[M,N] = A[M,K] . W[N,K]^T (+ bias[N]) (+ residual[m % res_rows, N]);  nn.Linear forward
 * (modules/attention.py:46-49,59; stage1/vqmodel.py:23,28; stage1/layers.py:149;
 * stage2/transformer.py:81,85,91).  A, W are `dtype`; bias/residual fp32 or NULL; out is
 * `out_dtype`.  res_rows lets one [tokens, N] table (a position embedding,
 * stage1/layers.py:108,146, stage2/transformer.py:82) be added to every image.  lda, ldw >= K; ldo >= N; with a residual
 * ldr >= N, and out may BE the residual (ldo == ldr, res_rows <= 0 or >= M): the fp32 stream updated in place. */
int pmhip_gemm(int dtype, const void* A, int lda, const void* W, int ldw, const float* bias,
               const float* residual, int ldr, int res_rows, void* out, int ldo, int out_dtype,
               int M, int N, int K, pmhip_stream stream);

/* SwiGLU first half (modules/mlp.py:27-30): out[M,Hp] = silu(x1) * x2 with
 * [x1|x2] = A . W12^T + b12.  W12p/b12p are the *packed* form: rows interleaved in groups of 16
 * (16 rows of x1, the matching 16 rows of x2, ...), hidden width zero-padded to Hp (mult. of 64). */
int pmhip_gemm_swiglu(int dtype, const void* A, int lda, const void* W12p, const float* b12p,
                      void* out, int ldo, int M, int Hp, int K, pmhip_stream stream);

/* Head-split projection (modules/attention.py:46-52): A[M,K] . W[nparts*inner,K]^T, no bias,
 * written per part as  Q -> [B,H,tokens,64] * q_scale ;  K -> [B,H,tokens_pad,64] ;
 * V -> transposed [B,H,64,tokens_pad].  M = B*tokens, inner = heads*64 (dim_head is 64).
 * The padding [tokens, tokens_pad) of K (rows) and V^T (columns) is left UNTOUCHED by every kernel that serves this entry point
 * (and by pmhip_gemm_heads_ln / _dh): what the caller put there stays there.  pmhip_attention never uses it (NaN included). */
int pmhip_gemm_heads(int dtype, const void* A, int lda, const void* W, int ldw, int M, int K,
                     int heads, int tokens, int tokens_pad, int nparts, const int* part_kinds_host,
                     void* const* part_outs_host, float q_scale, pmhip_stream stream);

/* ---- bf16 mode (the model-level default since round 3; PMHIP_HILO=0 restores the fp32 stream; DESIGN.md sections 4d, 4e): the
 * residual stream as a bf16 PAIR, and the LayerNorm folded into the GEMM that consumes it
 * (stage1/layers.py:54-58, stage2/transformer.py:44-49: x = f(LN(x)) + x, every projection preceded by a LayerNorm).
 * x = hi + lo with hi = bf16(x), lo = bf16(x - hi): two bf16 planes [M, D] -- the same 4 bytes per element as fp32 and, for a
 * stream built by adding bf16-GEMM outputs, the same accuracy (tools/residual_precision_probe.py: logits identical to the
 * fp32 stream to 5e-4, against +65 % error for a single bf16 plane).  What it buys: the hi plane IS bf16(x), the operand of
 * the next projection, so with  y = LN(x) = (x - mean) * rstd * gamma + beta  and
 *     y . W^T = rstd * (x . (gamma (.) W)^T) - rstd * mean * c + d,   c[n] = sum_k gamma[k] W[n,k],  d[n] = sum_k beta[k] W[n,k]
 * the projection multiplies hi by gamma-scaled weights and normalises in its epilogue; the separate LayerNorm pass over
 * the stream (read 4 B + write 2 B per element, 21 % of the GPU time of a decode step in round 2) is replaced by
 * pmhip_ln_coef, which reads the hi plane only.  Deterministic: no atomics. */

/* (hi, lo) <- split(A[M,K] . W[N,K]^T + bias + (res_hi + res_lo)[m % res_rows]); bf16 operands.  In place when the output
 * planes are the residual planes (out_hi == res_hi, out_lo == res_lo, ldo == ldr, no row modulo; see the memory contract above).
 * N, ldr, ldo multiples of 8; ldr >= N, ldo >= N. */
int pmhip_gemm_hilo(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res_hi,
                    const void* res_lo, int ldr, int res_rows, void* out_hi, void* out_lo, int ldo, int M, int N,
                    int K, pmhip_stream stream);
/* The same, and row_stats[M][N/64][2] = per row and per 64-column part (sum, sum of squares centred on the part's own mean) of
 * the NEW hi plane, written by the epilogue (N a multiple of 64): the LayerNorm folded into the next GEMM then needs no pass
 * over the plane -- pmhip_ln_coef_parts below instead of pmhip_ln_coef. */
int pmhip_gemm_hilo_stats(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res_hi,
                          const void* res_lo, int ldr, int res_rows, void* out_hi, void* out_lo, int ldo, int M, int N,
                          int K, float* row_stats, pmhip_stream stream);

/* Round 4, the CENTRED hi plane.  The folded LayerNorm normalises bf16(x); a row whose common offset is large against its spread
 * (trained transformers: massive activations, drifting row means) then loses 2^-9 |x| / std per element.  LayerNorm is blind to
 * a per-row shift, so this producer stores the pair of x - c, c = the row mean of the PREVIOUS hi plane read from `center_coef`
 * ([M][2] = the (rstd, -rstd * mean) pairs of pmhip_ln_coef / pmhip_ln_coef_parts for the LayerNorm in front of this branch;
 * NULL = no centring) plus `center_extra`, a launch-wide constant (the mean of `bias` over its N columns: the part of the new row
 * mean that is known in advance; a sudden common offset is then removed in the producer that introduces it).  `shift` ([M] floats, optional): running sum of the subtracted values for callers that need the absolute
 * x again (pmhip_unshift_hilo); shift_mode 1 = this producer opens the stream (shift <- 0), 2 = shift += c, 0 = untouched.
 * Everything else as pmhip_gemm_hilo_stats (row_stats may be NULL).  Replaces the same residual adds:
 * stage1/layers.py:55-56, stage2/transformer.py:45-48. */
int pmhip_gemm_hilo_center(const void* A, int lda, const void* W, int ldw, const float* bias, const void* res_hi,
                           const void* res_lo, int ldr, int res_rows, void* out_hi, void* out_lo, int ldo, int M, int N, int K,
                           float* row_stats, const float* center_coef, float center_extra, float* shift, int shift_mode,
                           pmhip_stream stream);
/* (hi, lo) <- split(hi + lo + shift[row]) in place: a centred stream back to the plain pair (D <= 1024, D % 4 == 0) */
int pmhip_unshift_hilo(void* x_hi, void* x_lo, const float* shift, int M, int D, pmhip_stream stream);
/* row operators on the pair (D a multiple of 4, <= 1024): LayerNorm of hi + lo -> f32 / bf16 (the unfolded path);
 * LayerNorm of an f32 row -> hi, lo; f32 -> hi, lo and back */
int pmhip_layernorm_hilo(const void* x_hi, const void* x_lo, const float* gamma, const float* beta, float eps,
                         void* out, int out_dtype, int M, int D, pmhip_stream stream);
int pmhip_layernorm_to_hilo(const float* x, const float* gamma, const float* beta, float eps, void* out_hi,
                            void* out_lo, int M, int D, pmhip_stream stream);
int pmhip_split_hilo(const float* x, void* out_hi, void* out_lo, int M, int D, pmhip_stream stream);
int pmhip_join_hilo(const void* x_hi, const void* x_lo, float* out, int M, int D, pmhip_stream stream);
/* coef[M][2] = (rstd, -rstd * mean) of the rows of the hi plane (two-pass, like the LayerNorm kernel) */
int pmhip_ln_coef(const void* x_hi, float eps, float* coef, int M, int D, pmhip_stream stream);
/* the same coefficients from pmhip_gemm_hilo_stats' partial statistics (D = 64 * nparts <= 1024): Chan's combination in part
 * order, deterministic; equal to pmhip_ln_coef to rounding (a few ulp of rstd) */
int pmhip_ln_coef_parts(const float* row_stats, int nparts, float eps, float* coef, int M, pmhip_stream stream);

typedef struct pmhip_lnfold {
    const float* coef;    /* [M][2]: (rstd, -rstd * mean) per row, from pmhip_ln_coef */
    const float* c;       /* [N]: sum_k of the (rounded) gamma-scaled weight row */
    const float* d;       /* [N]: sum_k beta[k] * W[n,k] */
    /* ABI 9, optional (parts NULL: coef is an input, as before).  parts = the [M][nparts][2] partial statistics
     * pmhip_gemm_hilo_stats left behind for this hi plane (nparts * 64 = K), eps the LayerNorm's: coef is then an OUTPUT of the
     * call as well -- written by the GEMM itself where a small launch computes its rows' coefficients in its prologue, by
     * pmhip_ln_coef_parts (launched by the call) otherwise; bit-identical either way. */
    const float* parts; int nparts; float eps;
} pmhip_lnfold;

/* Consumers: same arguments as pmhip_gemm (no residual) / pmhip_gemm_swiglu / pmhip_gemm_heads, with A = the hi plane,
 * W = the gamma-scaled weights and `ln` the fold descriptor.  Only shapes served by the 256x256 kernel
 * (pmhip_lnfold_supported; epi_kind 0 = plain, 1 = SwiGLU, 2 = head split; N counts the packed output rows). */
int pmhip_gemm_ln(int dtype, const void* A, int lda, const void* W, int ldw, const float* bias, void* out,
                  int ldo, int out_dtype, int M, int N, int K, const pmhip_lnfold* ln, pmhip_stream stream);
int pmhip_gemm_swiglu_ln(int dtype, const void* A, int lda, const void* W12p, const float* b12p, void* out,
                         int ldo, int M, int Hp, int K, const pmhip_lnfold* ln, pmhip_stream stream);
int pmhip_gemm_heads_ln(int dtype, const void* A, int lda, const void* W, int ldw, int M, int K, int heads,
                        int tokens, int tokens_pad, int nparts, const int* part_kinds_host,
                        void* const* part_outs_host, float q_scale, const pmhip_lnfold* ln,
                        pmhip_stream stream);
int pmhip_lnfold_supported(int dtype, int epi_kind, int M, int N, int K);

/* The logits GEMM of the MaskGIT step (stage2/transformer.py:91: to_logits) with the sampler's statistics from its epilogue (round 5):
 * out (f32) [M,N] = A . W^T + bias -- A, W as for pmhip_gemm, or, with `ln` not NULL, as for pmhip_gemm_ln -- and block_stats
 * [M][N/64][2] = (max, sum_j 2^((x_j - max) log2 e)) of every 64-column block of every row, computed from the values as they are
 * stored.  pmhip_sample_rows_stats then needs 8 bytes per block and the top-k blocks of a row instead of the row.  N % 64 == 0. */
int pmhip_gemm_softmax_stats(int dtype, const void* A, int lda, const void* W, int ldw, const float* bias, float* out, int ldo,
                             int M, int N, int K, const pmhip_lnfold* ln, float* block_stats, pmhip_stream stream);

/* softmax(Q K^T) V per (batch, head), no mask, no dropout (modules/attention.py:51-58; the same
 * maths as xformers.ops.memory_efficient_attention at :100).  Q is already scaled.  Layouts as
 * written by pmhip_gemm_heads.  out[B*Nq, heads*64] (`dtype`), head-major inside a row
 * ('(b h) n d -> b n (h d)', attention.py:58).  use_exp2 != 0: Q carries an extra log2(e) factor
 * and the kernel exponentiates with exp2. */
int pmhip_attention(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo,
                    int B, int heads, int Nq, int Nkv, int Nkv_pad, int use_exp2,
                    pmhip_stream stream);

/* Diagnostic of the bf16 kernel behind pmhip_attention (round 5).  Its fast path measures every probability against the
 * maximum of the query's first 32 keys and never looks at the running maximum again; a workgroup in which a probability
 * left the f32 range (scores more than 2^6 octaves above that reference; the softmax of modules/attention.py:53 itself
 * has no such limit) notices it when it normalises and runs again through its exact path, which raises the running
 * maximum at every half-tile.  *count = such workgroups on the current device since the last reset (synchronises the
 * device). */
int pmhip_attention_fallbacks(unsigned long long* count, int reset);

/* ---- any dim_head (modules/attention.py:27-33: inner_dim = dim_head * heads, scale = dim_head^-0.5).  The reference's
 * configs all use 64 and the tuned kernels above are built for it; these entry points forward to them when
 * dim_head == 64 and otherwise take a plain path: dim_head a multiple of 16 up to 128, heads*dim_head a multiple of 64.
 *   pmhip_gemm_heads_dh : the projection runs as an ordinary GEMM into `scratch` (f32 [M, nparts*heads*dim_head], caller
 *                         owned, unused when dim_head == 64) and a split kernel writes Q [B,H,tokens,dh] (* q_scale),
 *                         K [B,H,tokens_pad,dh] and V^T [B,H,dh,tokens_pad], rounding to `dtype` once.
 *   pmhip_attention_dh  : flash-style online softmax on the vector ALU, 4 lanes per query row. */
int pmhip_gemm_heads_dh(int dtype, const void* A, int lda, const void* W, int ldw, int M, int K, int heads, int dim_head,
                        int tokens, int tokens_pad, int nparts, const int* part_kinds_host,
                        void* const* part_outs_host, float q_scale, float* scratch, pmhip_stream stream);
int pmhip_attention_dh(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                       int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, pmhip_stream stream);

/* pmhip_attention_dh with a key count per IMAGE (a key-padding mask; new entry within ABI 11, nothing existing changes meaning):
 * kv_lens = DEVICE int32 [B]; image b attends to the keys [0, n_b) with n_b = min(max(kv_lens[b], 1), Nkv) -- the clamp is the
 * kernel's, an operator cannot validate device memory, and it keeps every read inside Nkv_pad.  Nkv stays the launch-wide upper
 * bound and Nkv_pad the layout: bases and row strides are those of pmhip_attention_dh.  Contract: the rows of image b equal, bit
 * for bit, pmhip_attention_dh called on that image alone with Nkv = n_b -- the same kernel body with the key count read once per
 * workgroup -- so K rows and V^T columns [n_b, Nkv_pad) of image b never reach a result, NaN included.  Any dim_head the _dh
 * entry serves (64 runs the tuned kernels); the workgroup shape of the bf16 kernel is chosen from B, heads and Nq only, never
 * from the lengths.  With every kv_lens[b] == Nkv the result is pmhip_attention_dh's.  kv_lens NULL is PMHIP_EINVAL. */
int pmhip_attention_lens(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                         int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const int32_t* kv_lens,
                         pmhip_stream stream);

/* pmhip_attention_dh with a key SET per QUERY (regional prompts; new entry within ABI 11, nothing existing changes meaning):
 *   key_seg    DEVICE uint8  [B, Nkv]: the segment 0..31 of image b's key k, or 255 = padding
 *   query_mask DEVICE uint32 [B, Nq] : bit s set = query q of image b attends to segment s
 * Key k takes part in query q's softmax iff key_seg[b,k] < 32 && (query_mask[b,q] >> key_seg[b,k]) & 1; every other key has weight
 * exactly 0 for that query.  Bases, strides, Nkv and Nkv_pad are those of pmhip_attention_dh; keys [Nkv, Nkv_pad) are padding.
 * Contract:
 *   - every query allows at least one key.  The model-level entries validate that where they own the arrays; this operator cannot
 *     validate device memory: a query with no allowed key yields a finite, unspecified row (zeros today), never a fault and never
 *     a read outside Nkv_pad or outside the two arrays
 *   - K rows and V^T columns with key_seg == 255 never reach a result, NaN included (their V^T columns are zeroed on chip; a
 *     probability of 0 alone would not do, 0 * NaN is NaN)
 *   - K rows and V^T columns with a segment 0..31 must be finite: a key allowed to some queries and denied to others contributes
 *     0 times a finite value where it is denied; a denied key never raises a query's running maximum, whatever its score
 *   - image b's rows do not depend on what else is in the batch
 *   - the padding value subsumes the per-image length: there is no kv_lens beside it
 * Any dim_head the _dh entry serves.  dim_head 64 runs the tuned kernels with the running maximum raised at every 32-key half-tile
 * (no lagged-max fast path, so pmhip_attention_fallbacks never counts these launches); the bf16 kernel runs 128 or 64 queries per
 * workgroup, chosen from B, heads and Nq only.  key_seg or query_mask NULL is PMHIP_EINVAL. */
int pmhip_attention_segments(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                             int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const uint8_t* key_seg,
                             const uint32_t* query_mask, pmhip_stream stream);

/* pmhip_attention_segments with a WEIGHT per key (prompt weights; new entries within ABI 11, nothing existing changes meaning;
 * DESIGN.md section 4w):
 *   key_bias DEVICE f32 [B, Nkv]: log(w[b,k]) in the kernel's score unit -- octaves when use_exp2, nats otherwise --, or -inf for
 *            w == 0.  pmhip_key_bias writes it from the weights.
 * Over the keys its segments allow, query q's probabilities are p[q,k] = w[k] exp(s[q,k]) / sum_j w[j] exp(s[q,j]): the bias is added
 * to the score (one f32 addition, in every 32-key half-tile, before the maximum is taken: the running maximum is a maximum over
 * s + bias).  An integer weight n is the key appearing n times.  key_seg, query_mask and every other argument are those of
 * pmhip_attention_segments.  Contract:
 *   - a key with bias -inf is a key with key_seg == 255, bit for bit: it never reaches a result, NaN in its K row and V^T column
 *     included, and never raises a running maximum; a key takes part in a query's softmax iff its segment is allowed AND its bias
 *     is above -inf
 *   - every bias == 0 gives pmhip_attention_segments's rows, bit for bit
 *   - every query allows at least one key with a bias above -inf (else: a finite, unspecified row, as there)
 *   - K rows and V^T columns of keys with a segment 0..31 and a bias above -inf must be finite; the biases are -inf or finite, and
 *     |bias| <= 20 octaves is what the model-level entries validate and the tests cover
 *   - image b's rows do not depend on what else is in the batch; there is no kv_lens beside the arrays
 * Any dim_head the _dh entry serves.  dim_head 64 runs the tuned kernels, every half-tile on the exact path as in the segmented form
 * (pmhip_attention_fallbacks never counts these launches); the bf16 kernel runs 128 or 64 queries per workgroup, chosen from B,
 * heads and Nq only, never from the arrays, bit-identical per 16-query tile.  The picked variant is pmhip_attention_pick_weighted, below.  key_seg,
 * query_mask or key_bias NULL is PMHIP_EINVAL. */
int pmhip_attention_weighted(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                             int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const uint8_t* key_seg,
                             const uint32_t* query_mask, const float* key_bias, pmhip_stream stream);
/* weights DEVICE f32 [n] -> bias DEVICE f32 [n]: 0 -> -inf, 1 -> exactly 0.0f, otherwise log2f(w), times ln 2 (one f32
 * multiplication) when use_exp2 == 0.  One asynchronous launch on `stream`, usable inside a captured graph; the two arrays do not overlap.
 * The range of w (0, or [2^-20, 2^20]) is the caller's to validate: this entry cannot read device memory on the host. */
int pmhip_key_bias(const float* weights, float* bias, int n, int use_exp2, pmhip_stream stream);

/* pmhip_attention_lens or pmhip_attention_segments for SOME images of the batch (regional prompts per slot; new entry within ABI
 * 11, nothing existing changes meaning):
 *   pick DEVICE uint8 [B]: the kind of every image;  want: the kind this launch serves (0..255)
 * Exactly one of kv_lens, or the pair key_seg + query_mask, is non-NULL and selects the form; the other arguments are those of the
 * entry it selects.  A workgroup of an image with pick[b] != want returns at once: it reads nothing of that image's Q, K, V^T,
 * length or segments (NaN there reaches nothing) and leaves EVERY byte of that image's rows of `out` as it found it.  An image
 * with pick[b] == want gets, bit for bit, the rows pmhip_attention_lens / pmhip_attention_segments writes for it on the same
 * inputs: same kernel text, same launch geometry, and the workgroup size chosen from B, heads and Nq only -- never from `pick` --,
 * so what an image computes does not depend on which images a launch serves.  Two launches, one per kind, fill one buffer.
 * A skipped image never counts in pmhip_attention_fallbacks; a served one of the kv_lens form takes the lagged-max fast path and
 * its exact re-run exactly as in pmhip_attention_lens.  pick NULL, both forms or none, or one of key_seg / query_mask without
 * the other: PMHIP_EINVAL. */
int pmhip_attention_pick(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                         int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const int32_t* kv_lens, const uint8_t* key_seg,
                         const uint32_t* query_mask, const uint8_t* pick, int want, pmhip_stream stream);

/* pmhip_attention_weighted for SOME images of the batch (prompt weights per slot; new entry within ABI 11, nothing existing
 * changes meaning): the arguments of pmhip_attention_weighted, then pick and want as in
 * pmhip_attention_pick.  The contract is that entry's: a workgroup of an image with pick[b] != want returns at once -- it reads
 * nothing of that image's Q, K, V^T, segments or biases (NaN there reaches nothing) and leaves EVERY byte of that image's rows of
 * `out` as it found it; an image with pick[b] == want gets, bit for bit, the rows pmhip_attention_weighted writes for it on the
 * same inputs (same kernel text, same launch geometry, 128 or 64 queries per workgroup in bf16 chosen from B, heads and Nq only,
 * never from `pick` or the arrays).  Three launches -- pmhip_attention_pick with kv_lens, pmhip_attention_pick with the key sets,
 * this entry --, one per kind, fill one buffer.  These launches never count in pmhip_attention_fallbacks.  pick, key_seg,
 * query_mask or key_bias NULL, or want outside 0..255: PMHIP_EINVAL. */
int pmhip_attention_pick_weighted(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads,
                                  int dim_head, int Nq, int Nkv, int Nkv_pad, int use_exp2, const uint8_t* key_seg,
                                  const uint32_t* query_mask, const float* key_bias, const uint8_t* pick, int want,
                                  pmhip_stream stream);

/* Cross-attention maps: the head-mean probabilities of one attention launch, materialised (new entry within ABI 11, nothing
 * existing changes meaning).  The flash kernels above never hold a row of P; this entry recomputes it from the
 * Q and K such a launch reads.  Q [B,H,Nq,dh] and K [B,H,Nkv_pad,dh] (`dtype`) have the layouts pmhip_gemm_heads(_dh) writes; Q is
 * already scaled and carries log2(e) when use_exp2 != 0.  maps DEVICE f32 [B, Nq, ldm], ldm >= Nkv.  For every image b, query q and
 * key k < Nkv:
 *     v = scale * (1 / heads) * sum_h p_h[q,k]          maps[b,q,k] = accumulate ? maps[b,q,k] + v : v
 * p_h is the softmax of the attention entry the nullable arrays select:
 *     all NULL                           pmhip_attention_dh
 *     kv_lens                            pmhip_attention_lens, with the same clamp to [1, Nkv]
 *     key_seg + query_mask               pmhip_attention_segments
 *     key_seg + query_mask + key_bias    pmhip_attention_weighted
 * Any other combination is PMHIP_EINVAL.  Contract:
 *   - excluded keys: a key that takes no part in a query's softmax -- behind the image's length, of a segment the query does not
 *     attend to, of segment 255, with bias -inf -- is written as exactly 0.0f, or left as it is under `accumulate`; NaN in the K row
 *     of such a key reaches nothing (it is masked by a select, never by arithmetic)
 *   - row sums: over the keys that take part, a row of one launch sums to `scale` within f32 rounding ((Nkv + heads + 74) 2^-23
 *     relative, plus the score error of the bound in tests/attnmap_ref.py)
 *   - memory: columns [Nkv, ldm) of every row and every byte outside `maps` are untouched; nothing is read outside Nkv_pad or the
 *     arrays (K rows at or behind Nkv are never read)
 *   - a query with no allowed key yields a finite, unspecified row (zeros today), as in pmhip_attention_segments
 *   - determinism: the sum over the heads runs in the fixed order h = 0 .. heads-1 inside one thread; there are no floating-point
 *     atomics; every element of `maps` is written by exactly one thread, once per launch; two launches on the same inputs agree bit
 *     for bit; image b's rows do not depend on what else is in the batch
 *   - precision: P stays f32, also in bf16 mode.  The product's bf16 kernel rounds P to bf16 for its P.V MFMA; the maps report the f32
 *     probabilities of the same bf16 Q and K, not those rounded values
 * Any dim_head the _dh entry serves, any Nkv (two passes over the context; registers and LDS do not depend on it), heads <= 64.  bf16
 * with dim_head 64 runs on MFMA (64 queries per workgroup, 16 per wave; Q and K 16-byte aligned); fp32 and every other dim_head run a
 * plain vector-ALU kernel, 4 lanes per query. */
int pmhip_attention_maps(int dtype, const void* Q, const void* K, float* maps, int ldm, int B, int heads, int dim_head, int Nq, int Nkv,
                         int Nkv_pad, int use_exp2, const int32_t* kv_lens, const uint8_t* key_seg, const uint32_t* query_mask,
                         const float* key_bias, float scale, int accumulate, pmhip_stream stream);

/* Cross-attention control: the edited pass of a prompt-to-prompt pair attends with probabilities blended from the source pass's (new
 * entry within ABI 11, nothing existing changes meaning).  The flash kernels above never hold a row of P, so
 * no form of theirs can blend two passes; this entry recomputes both softmaxes.  B pairs.  Qs [B,H,Nq,dh] and Ks [B,H,Ls_pad,dh] are
 * the source pass's, Qt, Kt [B,H,Lt_pad,dh] and Vt [B,H,dh,Lt_pad] the edited pass's (`dtype`), in the layouts pmhip_gemm_heads(_dh)
 * writes; both Q are already scaled and carry log2(e) when use_exp2 != 0.  out (`dtype`) [B*Nq, ldo], ldo >= heads * dim_head.
 *     row_map DEVICE int32 [B, Lt]: the source row of every target row, negative for none
 *     blend   DEVICE f32   [B, Lt]: in [0, 1]            gain DEVICE f32 [B, Lt]: finite and >= 0
 *     lens_s, lens_t DEVICE int32 [B] or NULL: the pair's key counts ns, nt, with the clamp of pmhip_attention_lens to [1, Ls] / [1, Lt];
 *                   NULL: Ls / Lt
 * For every pair b, head h, query q:
 *     ps = softmax over k < ns of Qs_h Ks_h^T           pt = softmax over j < nt of Qt_h Kt_h^T
 *     m = row_map[b,j];  has = 0 <= m < ns && blend[b,j] != 0
 *     P[q,j] = gain[b,j] * (has ? (1 - blend[b,j]) * pt[q,j] + blend[b,j] * ps[q,m] : pt[q,j])                    j < nt
 *     out[b*Nq + q, h*dh : (h+1)*dh] = sum_j P[q,j] * V_h[j,:]                  (no renormalisation, as in Hertz et al.)
 * Contract:
 *   - select, not arithmetic: a target key at or behind nt reaches nothing, NaN in its K row and V^T column included (the K row is
 *     never read; the MFMA kernel reads a V^T column only inside the 8-byte group of 4 keys that straddles nt and drops it by a select); where `has` is
 *     false no source score enters that key (a map entry at or behind ns is `none`); source rows at or behind ns are never read, so
 *     NaN there reaches nothing.  K rows below ns / nt and V^T columns below nt must be finite
 *   - the ranges of blend and gain are the caller's to validate (the model-level entry does): this operator cannot read device
 *     memory on the host.  Values outside them yield finite or non-finite rows, never a read or a write outside the stated extents
 *   - memory: nothing outside out's [B*Nq, heads*dim_head] extent under ldo is written; row_map, blend and gain are read in [B, Lt]
 *   - determinism: no floating-point atomics; every element of out is written by exactly one thread, once per launch; two launches
 *     on the same inputs agree bit for bit; pair b's rows do not depend on what else is in the batch
 *   - blend == 0 and gain == 1 everywhere is the softmax of pmhip_attention_lens on the edited pass, computed by other kernels: equal
 *     within the two entries' bounds (tests/control_ref.py), not bit for bit
 *   - precision: bf16 with dim_head 64 rounds P -- after blend and gain -- to bf16 for its P.V MFMA, as the product kernel does, and
 *     accumulates in f32; every other path keeps P in f32.  One rounding of out to `dtype`
 * Any dim_head the _dh entry serves, heads <= 64, B * heads <= 65535, any Ls and Lt (two passes over both contexts; registers do not
 * depend on them, and there is no LDS).  bf16 with dim_head 64 runs on MFMA (64 queries per workgroup, 16 per wave; Q and K 16-byte
 * aligned, Vt and out 8-byte aligned, Lt_pad and ldo multiples of 4); fp32 and every other dim_head run a plain vector-ALU kernel, 4
 * lanes per query.  A NULL operand or control array, or a shape outside the above: PMHIP_EINVAL before any launch. */
int pmhip_attention_control(int dtype, const void* Qs, const void* Ks, const void* Qt, const void* Kt, const void* Vt, void* out, int ldo,
                            int B, int heads, int dim_head, int Nq, int Ls, int Ls_pad, int Lt, int Lt_pad, int use_exp2,
                            const int32_t* row_map, const float* blend, const float* gain, const int32_t* lens_s, const int32_t* lens_t,
                            pmhip_stream stream);

/* Phrase score: where a prompt-to-prompt pair looks at a phrase, summed over the phrase's context rows and averaged over the heads
 * (new entry within ABI 11, nothing existing changes meaning).  The operands, layouts, lengths and control
 * arrays are those of pmhip_attention_control without Vt / out; row_map, blend and gain may be NULL, all three together: no control.
 *     w_s DEVICE f32 [B, Ls], w_t DEVICE f32 [B, Lt]: the phrase's row weights, finite and >= 0, typically 0 / 1
 *     score_s, score_t DEVICE f32 [B, Nq], contiguous
 * For every pair b and query q, with ps, pt, has and P exactly as pmhip_attention_control defines them (P = pt without control):
 *     vs = scale / heads * sum_h sum_{k < ns} w_s[b,k] * ps_h[q,k]        score_s[b,q] = accumulate ? score_s[b,q] + vs : vs
 *     vt = scale / heads * sum_h sum_{j < nt} w_t[b,j] * P_h[q,j]         score_t[b,q] = accumulate ? score_t[b,q] + vt : vt
 * Contract:
 *   - select, not arithmetic: a key at or behind the pair's length reaches nothing -- its K row and its weight are never read, NaN
 *     included; a map entry at or behind ns is `none`; a row of weight 0 takes part in the softmax and adds nothing.  K rows below
 *     ns / nt must be finite; the ranges of the weights, blend and gain are the caller's to validate (the model-level entry does)
 *   - memory: nothing outside the two [B, Nq] extents is written; w_s is read in [B, Ls], w_t and the control arrays in [B, Lt]
 *   - determinism: the sums over the heads (h = 0 .. heads-1) and the keys run in a fixed order; no floating-point atomics; every
 *     element is written by exactly one thread, once per launch; two launches on the same inputs agree bit for bit; pair b's rows
 *     do not depend on what else is in the batch
 *   - precision: P stays f32 in both dtypes -- the score reports the probabilities of the Q and K given, not the bf16-rounded
 *     values pmhip_attention_control feeds its P.V MFMA.  The bound is in tests/blend_ref.py
 * Shapes as pmhip_attention_control: any dim_head the _dh entry serves, heads <= 64, B * heads <= 65535, any Ls and Lt (two passes
 * over both contexts per head; registers do not depend on them, and there is no LDS).  bf16 with dim_head 64 runs on MFMA (64 queries
 * per workgroup, 16 per wave; Q and K 16-byte aligned); fp32 and every other dim_head run a plain vector-ALU kernel, 4 lanes per
 * query.  A NULL operand, weight or score array, a partly given control triple, or a shape outside the above: PMHIP_EINVAL before any
 * launch. */
int pmhip_attention_phrase_score(int dtype, const void* Qs, const void* Ks, const void* Qt, const void* Kt, int B, int heads, int dim_head,
                                 int Nq, int Ls, int Ls_pad, int Lt, int Lt_pad, int use_exp2, const int32_t* row_map, const float* blend,
                                 const float* gain, const int32_t* lens_s, const int32_t* lens_t, const float* w_s, const float* w_t,
                                 float* score_s, float* score_t, float scale, int accumulate, pmhip_stream stream);

/* The blend region of a pair from its two phrase scores: the rule of Pipeline.phrase_mask on both halves,
 * joined, then dilated.  score_s, score_t DEVICE f32 [B, g*g] (finite), mask_out DEVICE uint8 [B, g*g], 0 or 1:
 *     m_x[b,t] = score_x[b,t] >= threshold * max_t' score_x[b,t']        (one f32 product, an f32 compare)
 *     mask[b]  = dilate^grow (m_s[b] | m_t[b])                            a 3 x 3 maximum on the g x g grid, borders clipped
 * 0 < threshold <= 1, grow >= 0, 1 <= g <= 64, else PMHIP_EINVAL.  One workgroup per pair, the grid in LDS.  A maximum has no order
 * and the product is one rounding: given the same score bits the mask is exact.  An all-zero score row yields an all-true mask. */
int pmhip_phrase_region(const float* score_s, const float* score_t, uint8_t* mask_out, int B, int g, float threshold, int grow,
                        pmhip_stream stream);

/* The token blend under a region: mask DEVICE uint8 [B, N]; pred, merged DEVICE int64 [B, N], score DEVICE f32
 * [B, N], the _s arrays of the source half, the _t arrays of the edited half.  Where mask == 0 the three _t arrays take the _s arrays'
 * values; where mask != 0 they are untouched.  The _s arrays and the mask are read only; nothing else is written. */
int pmhip_blend_tokens(const uint8_t* mask, const int64_t* pred_s, const int64_t* merged_s, const float* score_s, int64_t* pred_t,
                       int64_t* merged_t, float* score_t, int B, int N, pmhip_stream stream);

/* torch.nn.LayerNorm over the last dim, eps inside the sqrt (stage1/layers.py:49,51,89,128;
 * stage2/transformer.py:37,39,41,62).  x fp32 [M,D] -> out (`out_dtype`). */
int pmhip_layernorm(const float* x, const float* gamma, const float* beta, float eps, void* out,
                    int out_dtype, int M, int D, pmhip_stream stream);

/* ---- the Flan-T5 encoder's own operators (new entries within ABI 11, nothing existing changes meaning).
 * The tower is the text encoder of modules/encoder.py:18-42; its arithmetic is Hugging Face's modeling_t5.py. */

/* T5LayerNorm: out[m,:] = weight * (x[m,:] * rsqrt(mean(x[m,:]^2) + eps)) -- no mean subtraction, no bias, statistics in f32.
 * x f32 [M,D], weight f32 [D], out `out_dtype` (f32, or bf16 rounded once) [M,D].  D % 4 == 0 and 4 <= D <= 4096 (a row is held
 * in registers and read once); any other D is PMHIP_EINVAL naming D.  An all-zero row gives zeros (eps > 0). */
int pmhip_rmsnorm(const float* x, const float* weight, float eps, void* out, int out_dtype, int M, int D, pmhip_stream stream);

/* T5's gated GELU (T5DenseGatedActDense with NewGELUActivation): out[m,j] = gelu_new(u[m,j]) * u[m,F+j] for j < F, with
 * gelu_new(x) = 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))).  u f32 [M, ldu >= 2F] -- the output of ONE GEMM against
 * [wi_0; wi_1] --, out `out_dtype` [M, ldo >= F].  F % 4 == 0; ldu, ldo multiples of 4 (16-byte accesses).  Columns [F, ldo) of out
 * are never written and columns [2F, ldu) of u never read.  Finite input gives finite output: where x^3 overflows the result is
 * x * u[m,F+j] (x > 0) or -0 * u[m,F+j] (x < 0), never NaN. */
int pmhip_geglu(const float* u, int ldu, void* out, int ldo, int out_dtype, int M, int F, pmhip_stream stream);

/* Self-attention with T5's relative-position bias (T5Attention, encoder, bidirectional), dim_head 64.  Layouts are those
 * pmhip_gemm_heads writes: Q [B,H,L,64] UNSCALED (T5 has no 1/sqrt(d): call pmhip_gemm_heads with q_scale = 1), K [B,H,L_pad,64],
 * V^T [B,H,64,L_pad], all `dtype`; out `dtype` [B*L, ldo >= heads*64], head-major inside a row, written in exactly its
 * B*L x heads*64 elements.
 *   rel_bias  DEVICE f32 [heads][2L-1], natural-log units: query q and key k of head h get rel_bias[h][(k - q) + (L - 1)] added to
 *             their score before the softmax.  T5's bucket depends on k - q only, so this table is all of the [H,L,L] bias, which
 *             is never materialised.  NULL is PMHIP_EINVAL.
 *   kv_lens   DEVICE int32 [B] or NULL: image b attends to the keys [0, n_b), n_b = min(max(kv_lens[b], 1), L) -- the clamp of
 *             pmhip_attention_lens; NULL: n_b = L.
 * Any L >= 1 is served (one wave per 16 queries walks the keys in blocks; L up to 2^20 by the entry's check).  L_pad >= L and a
 * multiple of 4; ldo a multiple of 4; Q, K, V^T 16-byte aligned.
 * bf16: Q K^T and P V on mfma_f32_16x16x32_bf16, the softmax in f32 with an exact running maximum that is subtracted before every
 * exponential (unscaled T5 scores reach the hundreds), P rounded to bf16 once.  f32: the same flow on the exact-f32 matrix core
 * (mfma_f32_16x16x4_f32), P not rounded.
 * Contract (that of the sibling forms): no atomics; two launches give the same bits; image b's rows do not depend on the rest of
 * the batch; K rows and V^T columns [L, L_pad) and behind n_b never reach a result, NaN included (the K rows are not read, the V^T
 * elements are replaced by 0 as they are loaded). */
int pmhip_attention_relbias(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int L,
                            int L_pad, const float* rel_bias, const int32_t* kv_lens, pmhip_stream stream);

/* ---- the OpenCLIP text tower's own operators (new entries within ABI 11, nothing existing changes meaning).
 * The tower is the text encoder of modules/encoder.py:45-104; its arithmetic is open_clip's ResidualAttentionBlock around
 * nn.MultiheadAttention. */

/* Causal self-attention, dim_head 64: out[q] = softmax_k(Q[q] . K[k]) V[k] over the keys k in [0, q], per (image, head).  Layouts are
 * those of pmhip_gemm_heads and pmhip_attention_relbias: Q [B,H,L,64] ALREADY SCALED, K [B,H,L_pad,64], V^T [B,H,64,L_pad], all
 * `dtype`; out `dtype` [B*L, ldo >= heads*64], head-major inside a row, written in exactly its B*L x heads*64 elements.
 * Any L in [1, 2^20]; L_pad >= L, a multiple of 4, at most 2^24; ldo a multiple of 4; Q, K, V^T 16-byte aligned, out 4-element
 * aligned.
 * One wave per 16 queries walks the keys [0, min(L, q0 + 16)) in blocks; blocks wholly above the diagonal are never visited.  The
 * softmax is in f32 with an exact running maximum subtracted before every exponential.  bf16: Q K^T and, for the keys below the
 * tile's first query, P V on mfma_f32_16x16x32_bf16 with P rounded to bf16 once (the denominator sums the unrounded P); f32: the
 * same flow on mfma_f32_16x16x4_f32.  The 16 keys of the diagonal tile are applied on the vector ALU with P in f32, because the
 * matrix core shares V^T among the queries of a tile.
 * Contract: no atomics; two launches give the same bits; image b's rows do not depend on the rest of the batch; row q depends on no
 * K row and no V^T column > q, NaN included, nor on the padding [L, L_pad). */
int pmhip_attention_causal(int dtype, const void* Q, const void* K, const void* Vt, void* out, int ldo, int B, int heads, int L,
                           int L_pad, pmhip_stream stream);

/* Head split of a projection that is already computed: U f32 [M, ldu >= nparts*heads*64] is the output of ONE ordinary pmhip_gemm
 * that added the projection's bias (nn.MultiheadAttention's in_proj_bias; pmhip_gemm_heads has no bias).  Part p is the columns
 * [p*heads*64, (p+1)*heads*64) and is written as pmhip_gemm_heads writes a part of kind part_kinds_host[p], rounded to `dtype` once:
 * Q -> [B,H,tokens,64] * q_scale ; K -> [B,H,tokens_pad,64] ; V -> transposed [B,H,64,tokens_pad].  M = B*tokens.  The f32 result
 * is the single f32 product U * q_scale (K and V: U itself), the bf16 result that product rounded to nearest even.  The padding
 * [tokens, tokens_pad) of K and V^T is left UNTOUCHED, and columns [nparts*heads*64, ldu) of U are never read.  part_kinds_host /
 * part_outs_host: HOST arrays of nparts (1..3) kinds and 16-byte aligned device pointers.  ldu a multiple of 4, U 16-byte aligned. */
int pmhip_split_heads(int dtype, const float* U, int ldu, int M, int heads, int tokens, int tokens_pad, int nparts,
                      const int* part_kinds_host, void* const* part_outs_host, float q_scale, pmhip_stream stream);

/* The GELUs of OpenCLIP's text towers on the f32 output of the c_fc GEMM (its bias already added): u f32 [M, ldu >= F] -> out
 * `out_dtype` (f32, or bf16 rounded once) [M, ldo >= F].
 *   kind 0   nn.GELU() (approximate='none'): 0.5 x (1 + erf(x / sqrt 2)), evaluated as 0.5 x erfc(-x sqrt(0.5)): no cancellation
 *            at negative x
 *   kind 1   open_clip's QuickGELU: x sigmoid(1.702 x), evaluated as x / (1 + exp(-1.702 x))
 * Finite input gives finite output in both kinds (far out: x, or -0).  F % 4 == 0; ldu, ldo multiples of 4 (16-byte accesses);
 * columns [F, ldo) of out are never written and columns [F, ldu) of u never read.  Any other kind is PMHIP_EINVAL. */
int pmhip_gelu(const float* u, int ldu, void* out, int ldo, int out_dtype, int M, int F, int kind, pmhip_stream stream);

/* Non-overlapping PxP patches of img[B,C,H,W] (fp32) as GEMM rows: out[B*(H/P)*(W/P), C*P*P],
 * column order (c, kh, kw) = the flattened Conv2d weight (stage1/layers.py:81-84,107). */
int pmhip_patchify(const float* img, void* out, int out_dtype, int B, int C, int H, int W, int P,
                   pmhip_stream stream);

/* 'b (h w) (p1 p2 c) -> b c (h p1) (w p2)' then clamp(lo,hi) (stage1/layers.py:150;
 * stage1/vqmodel.py:30).  y fp32 [B*(H/P)*(W/P), P*P*C] -> img fp32 [B,C,H,W].  The clamp is torch.clamp's: a NaN stays a
 * NaN (lo = -inf, hi = +inf copies every value). */
int pmhip_unpatchify_clamp(const float* y, float* img, int B, int C, int H, int W, int P, float lo,
                           float hi, pmhip_stream stream);

/* fp32 [M,K] -> `out_dtype` [M,Kpad], zero-padded columns (feeds K<64 projections). */
int pmhip_convert_pad(const float* in, int K, void* out, int out_dtype, int Kpad, int M,
                      pmhip_stream stream);

/* out[m,:] = x[m,:] + table[m % table_rows,:], all fp32 (x + position_embedding,
 * stage1/layers.py:108,146; stage2/transformer.py:82). */
int pmhip_add_rows(const float* x, const float* table, int table_rows, float* out, int M, int D,
                   pmhip_stream stream);

/* out = uncond + scale * (cond - uncond) over n fp32 elements (n % 4 == 0), fmaf per element; out may alias either input.
 * Guidance between the text-conditioned and the unconditional logits of one MaskGIT step: the reference trains for it by dropping
 * the text 10 % of the time (utils/trainer.py:379,387-388: `text = None` -> attn2 becomes a second self-attention,
 * modules/attention.py:47) but its own sampling (generate.py:159-181) never combines the two; SURVEY.md section 8(f) row 2. */
int pmhip_guidance_combine(const float* cond, const float* uncond, float scale, float* out, size_t n, pmhip_stream stream);
/* The same, and block_stats [n/64][2] = the softmax statistics (max, sum of exp) of every 64-element block of the result, for
 * pmhip_sample_rows_stats: rows must be contiguous and a multiple of 64 long (n % 64 == 0). */
int pmhip_guidance_combine_stats(const float* cond, const float* uncond, float scale, float* out, size_t n, float* block_stats,
                                 pmhip_stream stream);
/* The same two with the scale in DEVICE memory (new entry within ABI 11): the kernel loads scale_dev[0] once, wave-uniformly, in
 * front of its loop and then runs the loop of the entries above -- for the same value the logits and, with block_stats != NULL,
 * the statistics equal theirs bit for bit, in place (out == cond or uncond) as out of place.  block_stats NULL: the logits only.
 * Shape rules and NULL refusals are those of the scalar entries, given before anything is launched.  The VALUE cannot be checked
 * here: whoever wrote it to scale_dev checked it (the decode loop stages finite scales only).  A captured decode loop bakes in the
 * address, not the scale: this is what lets one graph serve every guidance schedule (pmhip_pipeline_generate_negative). */
int pmhip_guidance_combine_dev(const float* cond, const float* uncond, const float* scale_dev, float* out, size_t n,
                               float* block_stats /* or NULL */, pmhip_stream stream);

/* Row gather out[m,:] = table[ids[m],:] (nn.Embedding: stage1/quantize.py:41, generate.py:148-157),
 * table fp32 [V,E], ids int64, out `out_dtype` [M,Kpad] zero-padded. */
int pmhip_embed_rows(const float* table, const int64_t* ids, void* out, int out_dtype, int Kpad,
                     int M, int V, int E, pmhip_stream stream);

/* Codebook preparation, hoisted out of the per-call path: en = W / max(||W||,1e-12) row-wise and
 * sq[j] = sum(en[j]^2) (stage1/quantize.py:5-6,21,24-25). */
int pmhip_vq_prepare(const float* codebook, float* en, float* sq, int V, int E,
                     pmhip_stream stream);

/* VectorQuantizer.forward (stage1/quantize.py:18-38) on z fp32 [M,E] (the prev_quant output):
 * zn = l2norm(z); d = sum(zn^2) + sq - 2 zn.en^T; idx = first argmin; zq = en[idx];
 * z_out = zn + (zq - zn); loss = beta*mean((zq-zn)^2) + mean((zq-zn)^2).
 * The arithmetic order is fixed (sequential fmaf over E) and restated in oracle/vq_ref.c, so idx
 * is bit-exact against the oracle.  `scratch` >= pmhip_vq_scratch_bytes(M,V) bytes. */
size_t pmhip_vq_scratch_bytes(int M, int V);
int pmhip_vq_quantize(const float* z, const float* en, const float* sq, float beta, float* z_out,
                      int64_t* idx_out, float* loss_out, void* scratch, int M, int V, int E,
                      pmhip_stream stream);

/* Per-sample random masking of the latent sequence (Pipeline.random_masking, generate.py:78-110):
 * position i of sample b is KEPT iff fewer than len_keep positions of the sample have smaller noise
 * (ties: smaller index first, i.e. the order of a stable ascending argsort); masked positions get
 * mask_token.  z, x_out fp32 [B,N,E]; noise, mask_out fp32 [B,N] (mask: 0 keep, 1 masked);
 * len_keep = N - max(int(N*mask_ratio),1) is computed by the caller (generate.py:86-87).  0 <= len_keep <= N, N <= 16384
 * (a sample's noise and flags sit in 8 N bytes of dynamic LDS, up to 128 of a CU's 160 KiB). */
int pmhip_random_mask(const float* z, const float* noise, const float* mask_token, int len_keep,
                      float* x_out, float* mask_out, int B, int N, int E, pmhip_stream stream);

/* Masked label-smoothed cross entropy, forward only (Pipeline.loss, generate.py:112-125):
 * row_loss[m] = mask[m] * CE(logits[m,:], labels[m]; label_smoothing) with torch's definition
 * (1-eps)*nll + eps*mean_c(-log p_c); loss_out[0] = sum(row_loss) / sum(mask) (nan if nothing is
 * masked, as in the reference).  logits fp32 [M,V] with row stride ldl, labels int64 in [0,V). */
int pmhip_masked_ce(const float* logits, int ldl, const int64_t* labels, const float* mask,
                    float label_smoothing, float* row_loss, float* loss_out, int M, int V,
                    pmhip_stream stream);

/* One MaskGIT sampling pass over logits rows (generate.py:163-173 with helpers :29-46):
 * top-k filter, gumbel-argmax at `temperature`, confidence from the UNfiltered softmax, merge into
 * the previously masked positions.  noise: NULL -> counter-based Philox keyed by
 * (seed, step, row_base+row, column); else fp32 [M,V] uniform(0,1) samples (parity mode, the
 * reference's torch.zeros_like(t).uniform_(0,1), generate.py:41).
 * Outputs: pred[M] (all positions, what the image is decoded from, generate.py:165),
 * ids_out[M] = where(ids_in==mask_id, pred, ids_in), score[M] = is_mask ? 1-p[pred] : -1e5.
 * ids_out may alias ids_in.  Ties: (value desc, index asc).  1 <= topk <= V (V <= 16384); topk = V is the sampler without a
 * filter.  Which kernel runs depends on (V, topk) only: up to 8 with V % 64 == 0 the block-statistics kernel, up to 64 the row
 * kernel with one candidate per lane, above 64 (within ABI 11: a wider accepted range, nothing that was accepted changes by a
 * bit) the selection kernel, which keeps exactly the first topk elements of that order.  The noise of a (row, column) pair does
 * not depend on topk.  -inf logits are legal (they sort last); NaN is unspecified. */
int pmhip_sample_rows(const float* logits, int ldl, const int64_t* ids_in, int64_t mask_id,
                      int topk, float temperature, const float* noise, uint64_t seed,
                      uint32_t step, uint64_t row_base, int64_t* pred_out, int64_t* ids_out,
                      float* score_out, int M, int V, pmhip_stream stream);

/* The same step with a NUCLEUS (top-p) filter behind the top-k (new entries within ABI 11).  0 < top_p <= 1, finite (else
 * PMHIP_EINVAL); top_p == 1 is pmhip_sample_rows: the same kernel, the same bits.  Below 1, with K the first topk elements of
 * (value desc, column asc), w_i = exp(x_i - max), Z = sum of w over K and P = top_p * Z: element i of K is kept iff the mass of
 * the elements of K whose weight is strictly above w_i is below P.  A plateau of equal weights is kept or dropped whole, the
 * row's maximum is always kept, a weight that underflows to 0 never is.  The filter reads the RAW logits, as the top-k does: the
 * temperature acts in the draw only, and the confidence stays the unfiltered softmax of the drawn id.  The noise of a (row,
 * column) pair depends neither on topk nor on top_p.  One kernel serves every topk in 1..V (block statistics play no part);
 * which kernel runs depends on (V, topk, top_p < 1) only.  Sums are fp32 in a fixed order: an element whose mass above it lies
 * within 1e-4 Z of P may fall on either side of what exact arithmetic gives (tests/nucleus_ref.py). */
int pmhip_sample_rows_nucleus(const float* logits, int ldl, const int64_t* ids_in, int64_t mask_id, int topk, float top_p,
                              float temperature, const float* noise, uint64_t seed, uint32_t step, uint64_t row_base,
                              int64_t* pred_out, int64_t* ids_out, float* score_out, int M, int V, pmhip_stream stream);

/* The FORCED step (a new entry within ABI 11): nothing is drawn.  target int64 [M] (device) gives every
 * row its id, and the row is scored as a draw scores the id it produced:
 *   pred_out[r] = target[r];  ids_out[r] = ids_in[r] == mask_id ? target[r] : ids_in[r];
 *   score_out[r] = 1 - softmax(logits[r])[target[r]] where the position took the target, -1e5 where its id was given.
 * One wave per row, one read of the row, the normaliser of pmhip_sample_rows' row kernel expression for expression: for a row
 * whose target is the id a draw produced, the triple is bit-identical to that draw's wherever the draw ran on the row kernel
 * (8 < topk <= 64, or V % 64 != 0), the selection kernel (topk > 64) or the nucleus kernel (top_p < 1).  The block-statistics
 * kernel (topk <= 8, V % 64 == 0) rounds its confidence differently: there the scores agree to the last bits, not in them.
 * A target outside [0, V) -- the mask id included -- is never used as an index (the range test sits in front of the load): the
 * row is stored as an undrawn row, pred_out = ids_out = ids_in, score_out = -1e5.  The targets are device memory and are not
 * read on the host.  pred_out and score_out may be NULL; ids_out may alias ids_in; logits, ids_in (unless aliased) and target
 * are read only.  M > 0, 0 < V <= 16384, V % 4 == 0, ldl % 4 == 0, ldl >= V, else PMHIP_EINVAL naming the argument. */
int pmhip_sample_rows_forced(const float* logits, int ldl, const int64_t* ids_in, const int64_t* target, int64_t mask_id,
                             int64_t* pred_out, int64_t* ids_out, float* score_out, int M, int V, pmhip_stream stream);

/* The DIVERGENCE between two rows of logits (a new entry within ABI 11).  a, b fp32 [M, V], both with the
 * row stride ldl; they may be the same pointer.  Row r is SCORED iff ids is NULL or ids[r] == mask_id (ids int64 [M]: the
 * masked-position rule of the samplers).  With p = softmax(a[r]) and q = softmax(b[r]), each over its own row,
 *   kind 0 (tv)        d = 1/2 sum_i |p_i - q_i|                       in [0, 1]
 *   kind 1 (jeffreys)  d = sum_i (p_i - q_i) (log p_i - log q_i)       >= 0, = KL(p || q) + KL(q || p)
 * any other kind is refused.  A column that is -inf in both rows contributes nothing; a column that is -inf in exactly one row
 * makes jeffreys +inf and is an ordinary column under tv; a NaN anywhere in a scored row gives NaN for that row and no other.
 *                    accumulate == 0                        accumulate != 0
 *   scored row       acc[r] = d;  count[r] = 1              acc[r] += d;  count[r] += 1
 *   unscored row     acc[r] = 0;  count[r] = 0              neither is touched
 * acc fp32 [M], count int32 [M] or NULL.  The logits of an unscored row are never loaded: a NaN there reaches nothing and the launch
 * costs the scored rows' bytes.  Every element of a scored row is requested once; one writer per row, a fixed order of the sums,
 * no atomics: two launches give the same bits.  a == b row-wise gives exactly 0.0f under both kinds, and swapping a and b gives
 * the same bits (divergence.hip states the evaluation order that yields both).  a and b are read only and 16-byte aligned.
 * M > 0, 0 < V <= 16384, V % 4 == 0, ldl % 4 == 0, ldl >= V, else PMHIP_EINVAL naming the argument. */
int pmhip_logit_divergence(const float* a, const float* b, int ldl, const int64_t* ids, int64_t mask_id, int kind, float* acc,
                           int32_t* count, int accumulate, int M, int V, pmhip_stream stream);

/* The model's LIKELIHOOD of a given token (a new entry within ABI 11).  a (and b, or NULL) fp32 [M, V] with
 * the row stride ldl; target, and ids when given, int64 [M] in device memory, never read on the host.  Row r is SCORED iff
 * (ids is NULL or ids[r] == mask_id) and 0 <= target[r] < V.  The range test sits in front of any use of the target as an index: a
 * target outside the range -- the mask id included -- makes the row an unscored row (the rule of pmhip_sample_rows_forced).
 * The row that is scored: b NULL, x = a[r] (scale is ignored); b given, the guided logits x_i = b_i + scale * (a_i - b_i), formed at
 * load by the expression of pmhip_guidance_combine (a = cond, b = uncond), bit for bit: the combined tensor is neither written nor
 * re-read.  scale must be finite.  With t = target[r], m = max_i x_i and s = sum_i exp(x_i - m), a scored row yields
 *   lp  = (x_t - m) - log s             natural log; <= 0 exactly; -inf for a target column at -inf
 *   ent = log s + sum_i p_i (m - x_i)   the entropy of softmax(x); >= 0, exactly 0 for a row with one finite column; a -inf column adds 0
 *   rk  = #{ i : x_i > x_t, or x_i == x_t and i < t }   the target's place in the samplers' order (value descending, column
 *         ascending), exact: rk < k iff topk = k would have kept the token
 * A NaN anywhere in a scored row gives NaN lp and ent for that row and no other; its rk is unspecified.
 *                    accumulate == 0                                    accumulate != 0
 *   scored row       logp[r] = lp; entropy[r] = ent; rank[r] = rk;      logp[r] += lp; entropy[r] += ent; rank[r] += rk;
 *                    count[r] = 1                                       count[r] += 1
 *   unscored row     all four = 0                                       none is touched
 * logp fp32 [M]; entropy fp32 [M], rank int32 [M], count int32 [M], each or NULL.  The logits of an unscored row are never loaded:
 * a NaN there reaches nothing and the launch costs the scored rows' bytes.  Every element of a scored row is requested once (the
 * target's own logit a second time); one writer per row, a fixed order of the sums, no atomics: two launches give the same bits
 * (logprob.hip states the evaluation order).  a, b, ids and target are read only; a and b are 16-byte aligned.
 * M > 0, 0 < V <= 16384, V % 4 == 0, ldl % 4 == 0, ldl >= V, a / target / logp non-NULL, else PMHIP_EINVAL naming the argument, in
 * front of any launch. */
int pmhip_token_logprob(const float* a, const float* b, float scale, int ldl, const int64_t* ids, int64_t mask_id, const int64_t* target,
                        float* logp, float* entropy, int32_t* rank, int32_t* count, int accumulate, int M, int V, pmhip_stream stream);

/* The same step for a caller that holds the SOFTMAX STATISTICS of the rows' 64-column blocks (round 5): block_stats [M][V/64][2] =
 * (max, sum_j 2^((x_j - max) log2 e)) per block, as pmhip_gemm_softmax_stats / pmhip_guidance_combine_stats leave them behind.
 * For topk <= 8 the kernel reads the statistics (8 bytes per block) and the topk blocks with the largest maxima -- they contain
 * the topk largest elements -- instead of the whole row: 1 KiB + topk x 256 B instead of 32 KiB at V = 8192.
 * Same result, bit for bit, as pmhip_sample_rows on the same logits: for topk <= 8 and V % 64 == 0 that entry runs the same
 * kernel and derives the statistics from the stored row with the same arithmetic.  (topk > 8: the statistics are ignored; the
 * range is pmhip_sample_rows': 1 <= topk <= V, the selection kernel above 64.)
 * V % 64 == 0.  Reference: generate.py:163-173, as above. */
int pmhip_sample_rows_stats(const float* logits, int ldl, const float* block_stats, const int64_t* ids_in, int64_t mask_id,
                            int topk, float temperature, const float* noise, uint64_t seed, uint32_t step,
                            uint64_t row_base, int64_t* pred_out, int64_t* ids_out, float* score_out, int M, int V,
                            pmhip_stream stream);

/* Re-mask the num_mask least confident tokens of every image (generate.py:175-179):
 * ids[b, topk(scores[b], num_mask)] = mask_id.  Ties: (score desc, index asc). N <= 4096. */
int pmhip_remask(int64_t* ids, const float* scores, int num_mask, int64_t mask_id, int B, int N,
                 pmhip_stream stream);

/* ABI 11: per-IMAGE decode state.  One record per image of a batch, in DEVICE memory for the two operators below (the model-level
 * entry pmhip_pipeline_step_slots takes host records and stages them).  Every value the scalar entries above take once per call
 * -- seed, step, temperature, top-k, mask count, global image index -- is taken per image, so requests that differ share a batch. */
typedef struct pmhip_slot {      /* one per image of the batch, 32 bytes */
    uint64_t seed;               /* Philox key */
    uint64_t image_index;        /* global image index: the row counter is image_index * tokens + position */
    float    temperature;        /* this step's temperature, as the caller derived it */
    int32_t  topk;               /* 1..8 (1..V through the *_filter entries) */
    int32_t  num_mask;           /* this step's num_token_masked, >= 1 */
    uint32_t step;               /* Philox counter word; bit 31 set = slot idle */
} pmhip_slot;

/* pmhip_sample_rows / pmhip_sample_rows_stats with the scalars of row r taken from slots[r / tokens] (M = B * tokens rows, slots a
 * DEVICE array [B]): the same kernel body, arithmetic and order -- image b's rows equal, bit for bit, the scalar entry called on
 * that image alone with its slot's values and row_base = image_index * tokens.  Philox noise only.  An idle slot (bit 31 of step)
 * draws nothing: ids_out = ids_in, pred = ids_in, score = -1e5.  Served: the block-statistics kernel only, i.e. V % 64 == 0 and
 * every topk in 1..8 (what every decode-loop launch uses); block_stats may be NULL (derived from the stored rows). */
int pmhip_sample_rows_slots(const float* logits, int ldl, const float* block_stats /* or NULL */,
                            const int64_t* ids_in, int64_t mask_id, const pmhip_slot* slots, int tokens,
                            int64_t* pred_out, int64_t* ids_out, float* score_out, int M, int V, pmhip_stream stream);
/* THE SAMPLER FILTERS PER IMAGE (a new entry within ABI 11): pmhip_sample_rows_slots with slots[b].topk
 * anywhere in 1..V (V: no filter) and a nucleus mass per image, top_p_dev a DEVICE float [B] beside the records (NULL: every slot
 * 1; an idle slot's value is not looked at).  Which kernel serves a row is the rule of the scalar entries, per slot: top_p < 1 the
 * nucleus kernel, else topk <= 8 the block-statistics kernel, <= 64 the row kernel, above it the selection kernel.  Four launches
 * in that fixed order (block statistics, row, selection, nucleus), each serving the rows of its class only -- every row of
 * pred_out / ids_out / score_out is written by exactly one of them, an idle slot's by the first (ids_out = ids_in, pred = ids_in,
 * score = -1e5) -- so image b's rows equal, bit for bit, pmhip_sample_rows, pmhip_sample_rows_stats or pmhip_sample_rows_nucleus
 * called on that image alone with its slot's values and row_base = image_index * tokens.  Shapes as pmhip_sample_rows_slots: V %
 * 64 == 0, V <= 16384, M % tokens == 0, ldl >= V, ids_out == ids_in allowed; block_stats (read by the first launch only) may be
 * NULL.  The records are device memory and are not validated here: a caller keeps 1 <= topk <= V and 0 < top_p <= 1. */
int pmhip_sample_rows_slots_filter(const float* logits, int ldl, const float* block_stats /* or NULL */,
                                   const int64_t* ids_in, int64_t mask_id, const pmhip_slot* slots /* DEVICE [B] */,
                                   const float* top_p_dev /* DEVICE [B], or NULL: every slot 1 */, int tokens,
                                   int64_t* pred_out, int64_t* ids_out, float* score_out, int M, int V, pmhip_stream stream);
/* pmhip_remask with num_mask = slots[b].num_mask; the row of an idle slot is left untouched.  Same keys, order and threshold. */
int pmhip_remask_slots(int64_t* ids, const float* scores, const pmhip_slot* slots, int64_t mask_id,
                       int B, int N, pmhip_stream stream);

/* CHOICE TEMPERATURE (new entries within ABI 11): MaskGIT's perturbed re-masking.  pmhip_remask with the
 * key of image b, position i, score s = scores[b,i] replaced by, each line one fp32 operation, round to nearest:
 *   choice_t == 0:  s                           (pmhip_remask, bit for bit)
 *   s < 0:          s                           (a given id, score -1e5: no noise is drawn; given ids sort below every taken one
 *                                                and are re-masked only when num_mask exceeds the taken positions, in index order)
 *   otherwise:      ph = 1 - s;  conf = logf(fmaxf(ph, 2^-24));  g = -log(-log(u)) with both logs clamped at 1e-20 (the token
 *                   draw's gumbel);  key = -fmaf(choice_t, g, conf)
 * Order (key desc, index asc), threshold element num_mask - 1, every position at or above it masked: as pmhip_remask.
 * u: noise[b*N + i] (fp32 uniform(0,1), the parity hook) or, noise == NULL, Philox4x32-10 under `seed` at the counter
 * (grow_lo, grow_hi, 0xFFFFFFFF, step), grow = row_base + b*N + i, u = (x >> 8) * 2^-24.  No class column is 0xFFFFFFFF
 * (V <= 16384): the stream is disjoint from pmhip_sample_rows' under the same seed, step and rows.
 * choice_t is the STEP's value (a loop over T steps uses choice_temperature * (1 - (step+1)/T), 0 on the last step): finite,
 * 0 <= choice_t <= 1000 (every noisy key then stays above -1e5), else PMHIP_EINVAL before anything is launched. */
int pmhip_remask_choice(int64_t* ids, const float* scores, int num_mask, int64_t mask_id, int B, int N, float choice_t,
                        const float* noise /* [B,N] or NULL */, uint64_t seed, uint32_t step, uint64_t row_base,
                        pmhip_stream stream);
/* The per-image form: num_mask, seed, step and image_index (grow = image_index * N + i) from slots[b], choice_t from
 * choice_t_dev[b], a DEVICE float [B] parallel to the slot records (pmhip_slot stays 32 bytes).  Image b equals
 * pmhip_remask_choice on its row alone with these values and row_base = image_index * N; an image with choice 0 takes the
 * plain key; the row of an idle slot is left untouched.  Philox noise only. */
int pmhip_remask_choice_slots(int64_t* ids, const float* scores, const pmhip_slot* slots, const float* choice_t_dev,
                              int64_t mask_id, int B, int N, pmhip_stream stream);
/* A COUNT PER IMAGE (new entries within ABI 11): counts_dev is a DEVICE int32 [B].  The row of image b
 * equals, bit for bit, pmhip_remask (pmhip_remask_choice) called on that row alone with num_mask = counts_dev[b] and the noise at
 * row_base + b * N.  counts_dev[b] == 0 leaves row b untouched -- its workgroup leaves like an idle slot's; the entries above keep
 * their clamp to 1 -- and so does a negative entry; a count above N masks the row.  In place like pmhip_remask.  Null pointers,
 * bad shapes and a bad choice_t are PMHIP_EINVAL before anything is launched. */
int pmhip_remask_counts(int64_t* ids, const float* scores, const int32_t* counts_dev /* [B] */, int64_t mask_id, int B, int N,
                        pmhip_stream stream);
int pmhip_remask_choice_counts(int64_t* ids, const float* scores, const int32_t* counts_dev /* [B] */, int64_t mask_id, int B, int N,
                               float choice_t, const float* noise /* [B,N] or NULL */, uint64_t seed, uint32_t step, uint64_t row_base,
                               pmhip_stream stream);
/* SLOT RECORDS WITH A COUNT PER SLOT (new entries within ABI 11): the per-image forms above with counts_dev,
 * a DEVICE int32 [B] parallel to the slot records (pmhip_slot stays 32 bytes).  Row b equals, bit for bit,
 *   counts_dev[b] <  0:  pmhip_remask_slots / pmhip_remask_choice_slots on that row -- the record's num_mask with its clamp to 1;
 *   counts_dev[b] >  0:  pmhip_remask_counts / pmhip_remask_choice_counts on that row ALONE (B = 1) with num_mask = counts_dev[b],
 *                        the slot's seed and step, choice_t = choice_t_dev[b] and row_base = image_index * N; above N: the row;
 *   counts_dev[b] == 0, or the slot is idle:  its input -- the workgroup leaves before it touches the row; the count of an idle
 *                        slot is not looked at.
 * In place like pmhip_remask.  Null pointers and bad shapes are PMHIP_EINVAL before anything is launched.  The records and the
 * counts are device memory and are not validated here. */
int pmhip_remask_slots_counts(int64_t* ids, const float* scores, const pmhip_slot* slots, const int32_t* counts_dev /* [B] */,
                              int64_t mask_id, int B, int N, pmhip_stream stream);
int pmhip_remask_choice_slots_counts(int64_t* ids, const float* scores, const pmhip_slot* slots, const float* choice_t_dev,
                                     const int32_t* counts_dev /* [B] */, int64_t mask_id, int B, int N, pmhip_stream stream);

/* Pixel-side operators of the edit call.
 * pmhip_mask_tokens: pixel_mask uint8 [B,H,W], ids int64 [B, (H/patch) * (W/patch)] IN PLACE, counts_out int32 [B].  Token (r, c)
 * of image b is regenerated iff ANY pixel of its patch x patch block is non-zero: its id becomes mask_id; counts_out[b] = how many
 * tokens of image b are.  Every other id is left as it is; counts_out is written in exactly its B elements.
 * patch >= 1, H % patch == 0, W % patch == 0.
 * pmhip_composite: gen / orig / out fp32 [B,C,H,W], pixel_mask uint8 [B,H,W] broadcast over C: out = mask != 0 ? gen : orig,
 * element-wise.  out may alias gen (or orig): every element is read by the thread that writes it.
 * Null pointers and bad shapes are PMHIP_EINVAL before anything is launched. */
int pmhip_mask_tokens(const uint8_t* pixel_mask, int patch, int64_t* ids, int64_t mask_id, int32_t* counts_out, int B, int H, int W,
                      pmhip_stream stream);
int pmhip_composite(const float* gen, const float* orig, const uint8_t* pixel_mask, float* out, int B, int C, int H, int W,
                    pmhip_stream stream);

/* Per-image GUIDANCE: a record parallel to pmhip_slot, which stays 32 bytes; the ABI version stays 11 (new entries only). */
typedef struct pmhip_slot_guide { float scale; uint32_t on; } pmhip_slot_guide;   /* 8 bytes, one per image; on = 0: not guided */
/* `on` names what the image is guided AGAINST: 1 the pass without a context, 2 the negative context's pass
 * (pmhip_pipeline_step_slots_negative, pmhip_guidance_combine_slots_which).  The entries that predate the second kind
 * (pmhip_guidance_combine_slots, the pmhip_pipeline_step_slots_guided / _lens / _choice entries) keep reading any non-zero value as 1. */
#define PMHIP_GUIDE_OFF      0u
#define PMHIP_GUIDE_UNCOND   1u
#define PMHIP_GUIDE_NEGATIVE 2u

/* pmhip_guidance_combine(_stats) per image: cond / uncond / out fp32 [M, V] with contiguous rows, M = B * tokens, guides and slots
 * DEVICE arrays [B].  For an image that is active (bit 31 of slots[b].step clear) and has guides[b].on != 0, every row becomes
 * fmaf(scale_b, cond - uncond, uncond) and -- block_stats [M][V/64][2] given -- its block statistics are written: the same
 * per-element and per-block arithmetic in the same lane layout, so those rows equal, bit for bit, pmhip_guidance_combine(_stats)
 * called on that image alone with its scale.  The rows of an idle or unguided image are NEITHER READ NOR WRITTEN, in `out` and in
 * `block_stats`: in place on the cond tower's logits and statistics they stay the unguided step's inputs.  out may alias cond (or
 * uncond).  V % 64 == 0, M % tokens == 0; null pointers and bad shapes are PMHIP_EINVAL before anything is launched. */
int pmhip_guidance_combine_slots(const float* cond, const float* uncond, const pmhip_slot_guide* guides,
                                 const pmhip_slot* slots, int tokens, float* out, float* block_stats /* or NULL */,
                                 int M, int V, pmhip_stream stream);
/* The same for the images of ONE kind (a new entry within ABI 11): image b is combined iff it is active and guides[b].on == which
 * (which = 1 or 2, else PMHIP_EINVAL); its rows of `out` (and of `block_stats` when given) become
 * fmaf(scale_b, cond - other, other).  Every other image -- idle, unguided, or of the other kind -- is NEITHER READ NOR WRITTEN.
 * The selector is a workgroup-uniform compare in front of the same loop, so a combined image's rows equal, bit for bit,
 * pmhip_guidance_combine(_stats) called on that image alone; which = 1 over records whose `on` is 0 or 1 equals
 * pmhip_guidance_combine_slots.  Two launches with which = 1 and 2 and two different `other` planes touch disjoint images: this
 * is how a decode step guides some slots against no text and others against their negative text. */
int pmhip_guidance_combine_slots_which(const float* cond, const float* other, const pmhip_slot_guide* guides,
                                       const pmhip_slot* slots, int which, int tokens, float* out,
                                       float* block_stats /* or NULL */, int M, int V, pmhip_stream stream);

/* ------------------------------------------------------------------------------------------------
 * Model level.  Weight tables are filled by the host packer (paintmind_amd/engine.py) from the
 * reference's state_dict layout.
 * ---------------------------------------------------------------------------------------------- */

typedef struct pmhip_layer_weights {
    const float* ln1_g; const float* ln1_b;    /* norm1                                         */
    const void* wqkv;                          /* attn1 to_q|to_k|to_v rows, [3*inner, dim] T   */
    const void* wo; const float* bo;           /* attn1 to_out.0  [dim, inner] T, [dim]         */
    const float* lnx_g; const float* lnx_b;    /* stage 2 only: norm2 (else NULL)               */
    const void* wqkv2;                         /* stage 2 only: attn2 to_q|to_k|to_v            */
    const void* wo2; const float* bo2;         /* stage 2 only: attn2 to_out.0                  */
    const float* ln2_g; const float* ln2_b;    /* the norm in front of the FFN                  */
    const void* w12p; const float* b12p;       /* packed SwiGLU w12, [2*hidden_pad, dim] T      */
    const void* w3p; const float* b3;          /* w3 zero-padded in K, [dim, hidden_pad] T      */
    /* LayerNorm fold (bf16 mode; all NULL = not folded): gamma-scaled weights + the c / d vectors of pmhip_lnfold  */
    const void* wqkv_f; const float* qkv_c; const float* qkv_d;        /* norm1 into attn1 q|k|v               */
    const void* wqkv2_f; const float* qkv2_c; const float* qkv2_d;     /* stage 2: norm2 into attn2 q|k|v      */
    const void* w12p_f; const float* w12_c; const float* w12_d;        /* the FFN norm into packed w12         */
    /* centred hi plane (pmhip_gemm_hilo_center): mean over the columns of the three residual-producer biases -- what a producer
     * adds to EVERY row's mean, known before the row is computed (0 when unused)                                          */
    float bo_mean, bo2_mean, b3_mean;
} pmhip_layer_weights;

typedef struct pmhip_tower_cfg {
    int dim, depth, heads, hidden_pad;
    int dim_head;                              /* 0 means 64 (the reference's configs); see pmhip_attention_dh */
} pmhip_tower_cfg;

typedef struct pmhip_vqgan_cfg {
    int image_size, patch_size, channels;
    int n_embed, embed_dim;
    float beta;
    pmhip_tower_cfg enc, dec;
} pmhip_vqgan_cfg;

typedef struct pmhip_vqgan_weights {
    const void* patch_w;                       /* conv weight as [dim, C*P*P] T                 */
    const float* enc_pos;                      /* [tokens, dim]                                 */
    const float* pre_g; const float* pre_b;    /* encoder.norm_pre                              */
    const pmhip_layer_weights* enc_layers;     /* host array [enc.depth]                        */
    const void* prevq_w; const float* prevq_b; /* [embed_dim, dim] T                            */
    const float* codebook_n;                   /* pmhip_vq_prepare output, [n_embed, embed_dim] */
    const float* codebook_sq;                  /* [n_embed]                                     */
    const void* postq_w; const float* postq_b; /* [dim, 64] T (K zero-padded)                   */
    const float* dec_pos;
    const pmhip_layer_weights* dec_layers;
    const float* dn_g; const float* dn_b;      /* decoder.norm                                  */
    const void* proj_w; const float* proj_b;   /* [P*P*C, dim] T                                */
} pmhip_vqgan_weights;

typedef struct pmhip_vqgan pmhip_vqgan;

/* VQModel (stage1/vqmodel.py:7-44).  The tables are copied; the pointed-to weights are not. */
int pmhip_vqgan_create(pmhip_vqgan** out, int device, int dtype, const pmhip_vqgan_cfg* cfg,
                       const pmhip_vqgan_weights* w);
void pmhip_vqgan_destroy(pmhip_vqgan* h);
/* VQModel.encode (vqmodel.py:21-25): img fp32 [B,C,H,W] -> z fp32 [B,N,E], idx int64 [B,N], loss[1] */
int pmhip_vqgan_encode(pmhip_vqgan* h, const float* img, int B, float* z_out, int64_t* idx_out,
                       float* loss_out, pmhip_stream stream);
/* VQModel.decode (vqmodel.py:27-30): z fp32 [B,N,E] -> img fp32 [B,C,H,W] clamped to [-1,1] */
int pmhip_vqgan_decode(pmhip_vqgan* h, const float* z, int B, float* img_out, pmhip_stream stream);
/* VQModel.decode_from_indice (vqmodel.py:38-41) */
int pmhip_vqgan_decode_indices(pmhip_vqgan* h, const int64_t* idx, int B, float* img_out,
                               pmhip_stream stream);
/* Encoder.forward / Decoder.forward alone (stage1/layers.py:106-112,145-152); the decoder variant
 * takes the post_quant output x fp32 [B,N,dim] and returns the un-clamped image. */
int pmhip_vqgan_encoder_forward(pmhip_vqgan* h, const float* img, int B, float* x_out,
                                pmhip_stream stream);
int pmhip_vqgan_decoder_forward(pmhip_vqgan* h, const float* x, int B, float* img_out,
                                pmhip_stream stream);

typedef struct pmhip_s2_cfg {
    int tokens, embed_dim, n_embed, context_dim, context_dim_pad;  /* context_dim_pad: mult. of 64 */
    pmhip_tower_cfg tower;
} pmhip_s2_cfg;

typedef struct pmhip_s2_weights {
    const float* tok_table;                    /* [n_embed+1, embed_dim]: RAW codebook rows, then
                                                  mask_token (generate.py:148-157)              */
    const void* tokproj_w; const float* tokproj_b;   /* [dim, 64] T                            */
    const float* pos;                          /* [tokens, dim]                                 */
    const void* ctxproj_w;                     /* [dim, context_dim_pad] T, NULL when Identity  */
    const pmhip_layer_weights* layers;         /* host array [depth]                            */
    const float* norm_g; const float* norm_b;
    const void* logits_w; const float* logits_b;     /* [n_embed, dim] T                       */
    const void* logits_wf; const float* logits_c; const float* logits_d;   /* final norm folded into to_logits (or NULL) */
} pmhip_s2_weights;

typedef struct pmhip_s2 pmhip_s2;

/* CondTransformer (stage2/transformer.py:52-93) */
int pmhip_s2_create(pmhip_s2** out, int device, int dtype, const pmhip_s2_cfg* cfg,
                    const pmhip_s2_weights* w);
void pmhip_s2_destroy(pmhip_s2* h);
/* CondTransformer.forward (transformer.py:80-93): tokens fp32 [B,N,E]; context fp32 [B,L,ctx] or
 * NULL (then attn2 is a second self-attention, modules/attention.py:47); logits fp32 [B,N,V]. */
int pmhip_s2_forward(pmhip_s2* h, const float* tokens, const float* context, int L, int B,
                     float* logits_out, pmhip_stream stream);

/* Pipeline.sample (generate.py:159-181), one MaskGIT step on ids int64 [B,N] in place.
 * img_out may be NULL (skip the ViT decode of generate.py:165); pred_out/score_out may be NULL.
 * topk, here and in every pmhip_pipeline_* entry below that takes one as an argument (sample / generate, their _guided, _lens and
 * _choice forms): 1 <= topk <= n_embed, as pmhip_sample_rows serves it; topk = n_embed samples without a filter.  The slots
 * entries keep 1..8 per record (pmhip_pipeline_step_slots); pmhip_pipeline_step_slots_filter serves 1..n_embed per slot. */
int pmhip_pipeline_sample(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L,
                          int B, int topk, float temperature, int num_mask, const float* noise,
                          uint64_t seed, uint32_t step, uint64_t image_base, float* img_out,
                          int64_t* pred_out, float* score_out, pmhip_stream stream);

/* Pipeline.generate's loop body (generate.py:189-196) for T steps.  temps_host[T], nmask_host[T]
 * are the per-step temperature and num_token_masked the caller derived exactly as the reference
 * does (generate.py:191-193,175); decode_host[T] != 0 selects the steps whose image is produced,
 * written consecutively into imgs_out [n_decoded, B, C, H, W] (device; may be NULL when imgs_host
 * is given).  The context projection and the cross-attention K/V of the static context are
 * computed once (the reference recomputes them every step, transformer.py:84-85).
 * use_graph: bit flags.  PMHIP_GENERATE_GRAPH (1): the loop is a chain of hipGraphs, one per segment ending in a decoded step.
 * The request is IGNORED (eager loop, same bits) while per-kernel timing is on, for T > 64, and when the process runs with
 * AMD_DIRECT_DISPATCH=0, where graph replay is broken on ROCm 7.2 (tools/hwtests/graph_dispatch_mode.hip); bit 5 of
 * pmhip_s2_switches tells a caller that this process is in that mode.
 * PMHIP_GENERATE_CONCURRENT_LANES (2): the caller runs other micro-batches on other streams at the same time; the loop then never
 * defers a step's ViT decode to a side stream.  The deferral exists on the GRAPH path only (fork / join inside the captured
 * segments, for B * tokens <= 65536: one lane alone leaves the chip partly idle: +15 % at B = 8, +1.5 % at B = 64); the eager
 * loop decodes in line -- results are the same either way.
 * PMHIP_GENERATE_FROM_MASK (4; added within ABI 11 -- a new flag bit and one new entry point, nothing existing changes meaning, so
 * the version number stays): the loop starts from the all-mask state.  The library fills its working ids with the
 * mask id (n_embed) itself -- the content of `ids` on entry is ignored, `ids` is still written on return -- so a caller cannot
 * claim the state falsely.  With context == NULL (and hence no guidance) step 0 then runs NO tower: the input of that pass is the
 * same for every image and every call, so its logits are a function of the weights alone, which a handle never changes.  The
 * handle keeps the step-0 logits (and block statistics) of ONE image -- tokens x n_embed fp32 + tokens x n_embed/64 x 2 fp32:
 * 32 MiB + 1 MiB at vit-s sizes -- computed by the first flagged loop (its ordinary step-0 tower; image 0's rows are kept) and
 * sampled from by every later one, at any B, T, top-k, temperature and seed, eager or replayed (row r reads row r % tokens; ids,
 * Philox counters and scores stay per row).  Rows of different images never mix and the kernels are batch-invariant, so the
 * result is the unflagged loop's bit for bit (tests/test_gpu_step0.py); pmhip_s2_step0_shared counts fills and hits.  With a
 * context the flag only fills the ids.  While per-kernel timing is on the shortcut is OFF, like the graph request: bench.py
 * divides the work of ALL T tower passes by the measured family times, which a skipped pass would overstate by T / (T - 1).
 * imgs_host != NULL replaces the reference's `imgs.append(img.cpu())` (generate.py:195-196): decoded
 * image d is copied to imgs_host + d * host_stride (floats; the caller's PINNED buffer, so that a
 * lane can fill its rows of a [n_decoded, B_total, C, H, W] tensor) on copy_stream as soon as it is
 * complete, under the following steps.  There is no cross-stream wait on the device (a barrier parked
 * in the copy queue starves concurrent lanes): the CALL paces itself instead -- with imgs_host it
 * blocks the calling thread between segments (hipEventSynchronize on the image just finished, one
 * segment always queued ahead) and returns once the last copy is enqueued; concurrent lanes are
 * driven from one thread each.  The caller synchronises copy_stream before reading the host buffer.
 * copy_stream NULL: the copies are enqueued on `stream`. */
#define PMHIP_GENERATE_GRAPH 1
#define PMHIP_GENERATE_CONCURRENT_LANES 2
#define PMHIP_GENERATE_FROM_MASK 4
int pmhip_pipeline_generate(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context,
                            int L, int B, int T, const float* temps_host, const int* nmask_host,
                            const unsigned char* decode_host, int topk, uint64_t seed,
                            uint64_t image_base, float* imgs_out, int use_graph,
                            pmhip_stream stream, float* imgs_host, size_t host_stride,
                            pmhip_stream copy_stream);

/* The same two entry points with GUIDANCE (round 5; an extension behind an explicit argument):
 * every step runs the tower twice on the step's tokens -- with the context, and as the unconditional branch the reference
 * trains by dropping the text 10 % of the time (utils/trainer.py:379,387-388: context None, attn2 a second self-attention,
 * modules/attention.py:47) -- and samples from uncond + guidance_scale * (cond - uncond) (pmhip_guidance_combine); everything
 * after the logits is the reference's step (generate.py:161-179).  context must not be NULL.  The loop is graph-captured and
 * lane-able like pmhip_pipeline_generate (one executable graph per guidance_scale value); scale 0 reproduces the unconditional
 * step bit for bit, and the result equals the operator-level composition pmhip_s2_forward x 2 + pmhip_guidance_combine +
 * sampling bit for bit (tests/test_gpu_model.py). */
int pmhip_pipeline_sample_guided(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L,
                                 int B, int topk, float temperature, int num_mask, const float* noise,
                                 uint64_t seed, uint32_t step, uint64_t image_base, float* img_out,
                                 int64_t* pred_out, float* score_out, float guidance_scale,
                                 pmhip_stream stream);
int pmhip_pipeline_generate_guided(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context,
                                   int L, int B, int T, const float* temps_host, const int* nmask_host,
                                   const unsigned char* decode_host, int topk, uint64_t seed,
                                   uint64_t image_base, float* imgs_out, int use_graph,
                                   pmhip_stream stream, float* imgs_host, size_t host_stride,
                                   pmhip_stream copy_stream, float guidance_scale);

/* ABI 11: one MaskGIT step (pmhip_pipeline_sample without the image) in which every image carries its own decode state:
 * slots_host[B] (HOST records, validated here: an active slot needs 1 <= topk <= 8 and num_mask >= 1 -- the wider range of the
 * scalar entries stops here: a batch that mixes records at and above 8 would need a second sampling launch chosen per step) replace topk, temperature,
 * num_mask, seed, step and image_base.  The records travel through a pinned ring to device memory, from where the sampling and
 * re-masking kernels read them; the tower never mixes rows, so image b's pred / score / ids equal, bit for bit, those of the
 * scalar step run at the same B with slot b's values (idle slots still run through the tower; their ids stay as they are).
 * flags: PMHIP_SLOTS_KEEP_CONTEXT -- `context` is ignored and the cross K/V the previous slots call on this handle prepared are
 * reused (PMHIP_ESTATE when nothing was prepared, when another entry point prepared a context since, or when B or L differ).
 * PMHIP_SLOTS_GRAPH -- the step (tower + sampling + re-masking, a linear chain) is captured once per (B, L or no context) and
 * replayed: first call eager, second captures.  Every per-image value is read from device memory, so one graph serves every
 * schedule and every mix of requests.  The request is ignored exactly when PMHIP_GENERATE_GRAPH is (timing on,
 * AMD_DIRECT_DISPATCH=0): eager, same bits.  Context preparation always runs outside the graph.  n_embed % 64 == 0.
 * pred_out [B,N] / score_out [B,N] may be NULL. */
#define PMHIP_SLOTS_GRAPH        1   /* replay a captured step */
#define PMHIP_SLOTS_KEEP_CONTEXT 2   /* reuse the cross K/V the previous slots call on this handle prepared */
int pmhip_pipeline_step_slots(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B,
                              const pmhip_slot* slots_host, int flags,
                              int64_t* pred_out, float* score_out, pmhip_stream stream);

/* The same step with per-image GUIDANCE: guides_host[B] (HOST records, may be NULL) travel beside the slot records through the
 * same pinned ring.  An active slot with on != 0 samples from uncond + scale * (cond - uncond) like pmhip_pipeline_sample_guided
 * with its own scale; it needs a finite scale and a context (L > 0, also under PMHIP_SLOTS_KEEP_CONTEXT), otherwise PMHIP_EINVAL
 * ("guidance needs a context") and nothing runs.  guides_host == NULL, or no ACTIVE slot guided: exactly
 * pmhip_pipeline_step_slots -- one tower pass, the same graph.  Otherwise a linear chain: the tower with the context (the logits
 * GEMM leaves the block statistics), the tower without it, pmhip_guidance_combine_slots in place on the first tower's logits and
 * statistics, the slots sampling tail.  An unguided slot beside a guided one keeps the first tower's rows untouched, so it
 * computes what it computes in pmhip_pipeline_step_slots, bit for bit; it still runs through the second tower (no compaction).
 * PMHIP_SLOTS_GRAPH: that chain is captured once per (B, L) under a key of its own; the scales are read from device memory, so
 * one graph serves every mix of scales.  Ignored when pmhip_pipeline_step_slots ignores it. */
int pmhip_pipeline_step_slots_guided(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B,
                                     const pmhip_slot* slots_host, const pmhip_slot_guide* guides_host, int flags,
                                     int64_t* pred_out, float* score_out, pmhip_stream stream);

/* Per-image CONTEXT LENGTHS (new entries within ABI 11, following pmhip_slot_guide: nothing existing changes meaning).  The model-
 * level entries above attend to all L rows of every image's context, padding included (the reference's behaviour with its T5
 * embedder: padding="max_length", no mask).  The *_lens entries take ctx_lens_host, a HOST int32 [B]: image b's cross-attention
 * sees the context rows [0, len_b) only.  Contract: rows [len_b, L) of image b's context never reach a result, NaN included, and
 * image b computes what it computes at the same B with any other lengths beside it.  ctx_lens_host == NULL: every image uses L --
 * exactly the entry without the suffix, the same kernels and the same graphs.
 *   - the lengths are validated before anything is launched: 1 <= len_b <= L, else PMHIP_EINVAL with a message naming the image;
 *     lengths without a context are PMHIP_EINVAL
 *   - they travel like the slot records: pinned ring -> copy kernel -> a handle-owned device array, from where the cross-attention
 *     launch (pmhip_attention_lens) reads them.  Captured graphs bake in that array, not the lengths: one graph per (B, L) serves
 *     every mix of lengths (a key of its own beside the unmasked graph's, since the kernel form differs)
 *   - the context projection and the cross K/V still cover all B * L rows; self-attention launches and the unconditional pass of a
 *     guided step never see lengths
 *   - PMHIP_SLOTS_KEEP_CONTEXT keeps the cross K/V only: every slots call brings its own lengths (or NULL), so a step in which only
 *     the lengths changed needs no new context
 * guided != 0: the entry is the _guided one with guidance_scale; guided == 0: guidance_scale is ignored.
 * pmhip_pipeline_step_slots_lens is pmhip_pipeline_step_slots_guided (guides_host may be NULL) with lengths. */
int pmhip_s2_forward_lens(pmhip_s2* h, const float* tokens, const float* context, int L, int B,
                          const int32_t* ctx_lens_host, float* logits_out, pmhip_stream stream);
int pmhip_pipeline_sample_lens(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                               const int32_t* ctx_lens_host, int topk, float temperature, int num_mask, const float* noise,
                               uint64_t seed, uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                               float* score_out, int guided, float guidance_scale, pmhip_stream stream);
int pmhip_pipeline_generate_lens(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                 const int32_t* ctx_lens_host, int T, const float* temps_host, const int* nmask_host,
                                 const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                 float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                 pmhip_stream copy_stream, int guided, float guidance_scale);
int pmhip_pipeline_step_slots_lens(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B,
                                   const int32_t* ctx_lens_host, const pmhip_slot* slots_host,
                                   const pmhip_slot_guide* guides_host, int flags, int64_t* pred_out, float* score_out,
                                   pmhip_stream stream);

/* CHOICE TEMPERATURE at the model level (new entries within ABI 11): the *_lens entries with the re-masking launch replaced by
 * its choice form (pmhip_remask_choice above); nothing else of the step changes, so it composes with guidance, context lengths,
 * lanes, PMHIP_GENERATE_FROM_MASK and PMHIP_SLOTS_KEEP_CONTEXT.  A NULL or all-zero choice argument runs exactly the *_lens
 * entry: the same kernels and the same captured graphs.  Values are validated before anything is launched (finite, in [0, 1000]).
 *   - pmhip_pipeline_sample_choice: choice_t is this step's value; choice_noise [B,N] (or NULL: Philox under seed / step /
 *     image_base, column word 0xFFFFFFFF) the uniforms of the re-masking keys
 *   - pmhip_pipeline_generate_choice: ctemps_host [T], one value per step.  With the graph flag the loop is captured under a key of
 *     its own and its re-masking launches read the values from the device parameter block: one graph serves every schedule
 *   - pmhip_pipeline_step_slots_choice: choice_host [B], one value per slot (idle slots are not looked at).  The values travel in the
 *     ring entry of the slot and guide records to a handle-owned device array; a step with a non-zero value has a graph key of
 *     its own, and one graph serves every mix of values */
int pmhip_pipeline_sample_choice(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                 const int32_t* ctx_lens_host, int topk, float temperature, int num_mask, const float* noise,
                                 uint64_t seed, uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                 float* score_out, int guided, float guidance_scale, float choice_t,
                                 const float* choice_noise /* [B,N] or NULL */, pmhip_stream stream);
int pmhip_pipeline_generate_choice(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                   const int32_t* ctx_lens_host, int T, const float* temps_host, const int* nmask_host,
                                   const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                   float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                   pmhip_stream copy_stream, int guided, float guidance_scale,
                                   const float* ctemps_host /* [T] or NULL */);
int pmhip_pipeline_step_slots_choice(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B,
                                     const int32_t* ctx_lens_host, const pmhip_slot* slots_host,
                                     const pmhip_slot_guide* guides_host, const float* choice_host /* [B] or NULL */, int flags,
                                     int64_t* pred_out, float* score_out, pmhip_stream stream);

/* NUCLEUS FILTER at the model level (new entries within ABI 11): the *_choice entries with `top_p`, the token draw's nucleus mass
 * (pmhip_sample_rows_nucleus above: 0 < top_p <= 1, validated before anything is launched), one value for the batch and, in the
 * loop, for every step.  top_p == 1 runs exactly the *_choice entry: the same kernels and the same captured graphs.  Below 1 the
 * sampling launch is the nucleus kernel and nothing else of the step changes, so it composes with guidance, context lengths,
 * choice temperatures, lanes and PMHIP_GENERATE_FROM_MASK; with the graph flag top_p is a kernel argument of the captured loop,
 * like topk: one graph per value.  The slots entries have no top_p: a pmhip_slot record carries none
 * (pmhip_pipeline_step_slots_filter takes one per slot beside the records). */
int pmhip_pipeline_sample_nucleus(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                  const int32_t* ctx_lens_host, int topk, float temperature, int num_mask, const float* noise,
                                  uint64_t seed, uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                  float* score_out, int guided, float guidance_scale, float choice_t,
                                  const float* choice_noise /* [B,N] or NULL */, float top_p, pmhip_stream stream);
int pmhip_pipeline_generate_nucleus(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                    const int32_t* ctx_lens_host, int T, const float* temps_host, const int* nmask_host,
                                    const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                    float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                    pmhip_stream copy_stream, int guided, float guidance_scale,
                                    const float* ctemps_host /* [T] or NULL */, float top_p);

/* NEGATIVE PROMPT and GUIDANCE SCHEDULE at the model level (new entries within ABI 11): the *_nucleus entries with
 *   - neg_context fp32 [B, Ln, context_dim] (device), Ln >= 1, and neg_lens_host, a HOST int32 [B] or NULL: the second tower of a
 *     guided step attends to THIS context instead of running without one -- the step samples from neg + scale * (cond - neg).
 *     The handle keeps a second set of cross K/V for it (workspace, device length array and ring staging of its own), prepared
 *     once per call like the context's; Ln need not equal L.  The lengths obey the *_lens contract: rows [len_b, Ln) of image b's
 *     negative context never reach a result, NaN included
 *   - (generate only) gscales_host, a HOST float [T] or NULL: step t combines with gscales_host[t]; the scalar guidance_scale is
 *     then ignored.  The scales travel with the temperatures in the device parameter block, and every combine launch of such a
 *     loop -- eager, captured or replayed -- is pmhip_guidance_combine_dev on the address of its step's scale: the loop has a graph
 *     key of its own and ONE graph serves every schedule.  T <= 128 with a schedule
 * neg_context == NULL (and gscales_host == NULL) runs exactly the *_nucleus entry: the same kernels and the same captured graphs;
 * in particular the scalar-scale loop keeps its one graph per guidance_scale value.  A negative context adds a component with
 * Ln (and whether lengths came) to the graph key.  The step with a negative context equals the operator-level composition
 * pmhip_s2_forward_lens(context) + pmhip_s2_forward_lens(neg_context) + pmhip_guidance_combine + sampling bit for bit; a loop
 * whose schedule is one value T times equals the scalar-scale loop bit for bit; with neg_context the same rows and lengths as
 * context the result is the UNGUIDED step's for every scale (cond - neg is exactly 0).  A step whose scale is 0 still runs both
 * towers.  Everything composes with context lengths, choice temperatures, the nucleus filter, lanes and the deferred decode
 * like the entries these extend.
 * Validated before anything is launched (PMHIP_EINVAL, ids untouched): a negative context or a schedule needs guided != 0 and a
 * context; Ln >= 1; 1 <= neg_len_b <= Ln (the message names the image); neg_lens_host without neg_context; every scale finite.
 * A later call through any model-level entry that brings no negative context drops the set: nothing runs against a stale one. */
int pmhip_pipeline_sample_negative(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                   const int32_t* ctx_lens_host, int topk, float temperature, int num_mask, const float* noise,
                                   uint64_t seed, uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                   float* score_out, int guided, float guidance_scale, float choice_t,
                                   const float* choice_noise /* [B,N] or NULL */, float top_p,
                                   const float* neg_context /* [B,Ln,context_dim] or NULL */, int Ln,
                                   const int32_t* neg_lens_host /* [B] or NULL */, pmhip_stream stream);
int pmhip_pipeline_generate_negative(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                     const int32_t* ctx_lens_host, int T, const float* temps_host, const int* nmask_host,
                                     const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                     float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                     pmhip_stream copy_stream, int guided, float guidance_scale,
                                     const float* ctemps_host /* [T] or NULL */, float top_p,
                                     const float* neg_context /* [B,Ln,context_dim] or NULL */, int Ln,
                                     const int32_t* neg_lens_host /* [B] or NULL */, const float* gscales_host /* [T] or NULL */);

/* THE EDIT LOOP (new entry within ABI 11): pmhip_pipeline_generate_negative with three changes.
 *   - nmask_img_host, a HOST int32 [T][B], replaces nmask_host: step t re-masks nmask_img_host[t * B + b] positions of image b
 *     (the counts form of the re-masking kernel, its choice form when a choice temperature is active); 0 leaves the image's ids
 *     as the step merged them.  The table travels through pinned memory into a handle-owned device table at a fixed address:
 *     a captured loop bakes in the address, never the counts, so one graph per (B, L, T, topk, top_p, ...) serves every set of masks
 *   - a decoded step decodes the MERGED ids -- where(ids == mask, pred, ids), taken before that step's re-masking -- instead of
 *     the predictions at all positions: a position whose id the caller gave decodes from that id
 *   - the loop starts from the caller's ids: PMHIP_GENERATE_FROM_MASK is refused, there is no shared step 0
 * Everything else -- tower, statistics, sampler choice, guidance (scalar or per step), negative context, context lengths, choice
 * temperatures, eager or captured under a graph key of its own -- is that entry's.
 * Validated before anything is launched (PMHIP_EINVAL, ids untouched): what that entry validates, and every table entry in
 * 0 .. tokens (the message names step and image). */
int pmhip_pipeline_generate_edit(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                 const int32_t* ctx_lens_host, int T, const float* temps_host,
                                 const int32_t* nmask_img_host /* [T][B] */, const unsigned char* decode_host, int topk, uint64_t seed,
                                 uint64_t image_base, float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host,
                                 size_t host_stride, pmhip_stream copy_stream, int guided, float guidance_scale,
                                 const float* ctemps_host /* [T] or NULL */, float top_p,
                                 const float* neg_context /* [B,Ln,context_dim] or NULL */, int Ln,
                                 const int32_t* neg_lens_host /* [B] or NULL */, const float* gscales_host /* [T] or NULL */);

/* NEGATIVE PROMPT PER SLOT (new entries within ABI 11): pmhip_pipeline_step_slots_choice with a negative
 * context neg_context fp32 [B, Ln, context_dim] (device, or NULL) and neg_lens_host, a HOST int32 [B] or NULL.  Through THIS entry
 * guides_host[b].on names what slot b is guided against: 0 not guided, 1 the pass without a context, 2 the negative context --
 * slot b then samples from neg_b + scale_b * (cond_b - neg_b), like pmhip_pipeline_sample_negative on that image.  The host
 * decides the tower passes of the step from the ACTIVE slots:
 *   1. the tower with the context, always (its logits GEMM leaves the block statistics);
 *   2. the tower without a context iff a slot has on == 1, then pmhip_guidance_combine_slots_which(which = 1) in place;
 *   3. the tower against the negative set iff a slot has on == 2, then the same with which = 2.
 * Passes 2 and 3 write the same second logits plane one after the other -- a linear chain, no third plane -- and the two combines
 * touch disjoint images, so an unguided slot keeps the first tower's rows and every slot computes, bit for bit, what it computes
 * alone.  A step without pass 3 runs the launches and the captured graph of pmhip_pipeline_step_slots_choice; one with it has a
 * graph key that adds the pass set, Ln and whether negative lengths came.
 * The negative K/V are prepared eagerly, outside any graph, in the handle's second set (as for pmhip_pipeline_sample_negative).
 * flags: PMHIP_SLOTS_KEEP_NEGATIVE -- neg_context is ignored and the negative K/V the PREVIOUS slots call on this handle prepared
 * (or kept) are reused, also across the preparation of a new context; PMHIP_ESTATE when there are none (no slots call prepared
 * any, the previous one neither brought nor kept them, another entry point ran since) or when B or Ln differ.  A call that
 * neither brings nor keeps a negative context drops the set.  Lengths are staged by every call that brings them, also under the
 * keep flag; NULL: every slot attends to all Ln rows.
 * Validated before anything is staged or launched (PMHIP_EINVAL, ids untouched): on in {0, 1, 2}; on == 2 needs a negative set,
 * given or kept, and a context; Ln >= 1; 1 <= neg_len_b <= Ln for every b (the message names the slot); neg_lens_host without a
 * negative set; every scale of a guided slot finite. */
#define PMHIP_SLOTS_KEEP_NEGATIVE 4  /* reuse the negative cross K/V the previous slots call on this handle prepared */
int pmhip_pipeline_step_slots_negative(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B,
                                       const int32_t* ctx_lens_host, const pmhip_slot* slots_host,
                                       const pmhip_slot_guide* guides_host, const float* choice_host /* [B] or NULL */,
                                       const float* neg_context /* [B,Ln,context_dim] or NULL */, int Ln,
                                       const int32_t* neg_lens_host /* [B] or NULL */, int flags,
                                       int64_t* pred_out, float* score_out, pmhip_stream stream);

/* THE SAMPLER FILTERS PER SLOT (new entries within ABI 11): pmhip_pipeline_step_slots_negative, the widest
 * slots entry, with the wider sampler.  Through THIS entry an active slot may carry 1 <= topk <= n_embed (n_embed: no filter) and
 * a nucleus mass top_p_host[b], finite and in (0, 1] (top_p_host a HOST float [B], or NULL: every slot 1); idle slots are not
 * looked at.  Validated before anything is staged or launched (PMHIP_EINVAL, ids untouched; the message names the slot).  The five
 * entries above keep their 1..8 per record.
 * When every active slot is served by the block-statistics kernel (top_p == 1 and topk <= 8) the call runs exactly
 * pmhip_pipeline_step_slots_negative: the same launches, the same graph key, the same captured graph.  Otherwise the sampling
 * tail is the four launches of pmhip_sample_rows_slots_filter; the tower passes, the combines, the re-masking and the choice
 * temperature stay as they are.  top_p travels in the pinned-ring entry of the records, behind the choice temperatures (an idle
 * slot's is 1), into a handle-owned device array; with PMHIP_SLOTS_GRAPH the chain form has one further graph key, and as every
 * record value and top_p are read from device memory, that one graph serves every mix of classes and values.  A slot computes,
 * bit for bit, what pmhip_pipeline_sample / _nucleus computes for that image alone with its values. */
int pmhip_pipeline_step_slots_filter(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B,
                                     const int32_t* ctx_lens_host, const pmhip_slot* slots_host,
                                     const pmhip_slot_guide* guides_host, const float* choice_host /* [B] or NULL */,
                                     const float* neg_context /* [B,Ln,context_dim] or NULL */, int Ln,
                                     const int32_t* neg_lens_host /* [B] or NULL */, const float* top_p_host /* [B] or NULL */,
                                     int flags, int64_t* pred_out, float* score_out, pmhip_stream stream);
/* Steps pmhip_pipeline_step_slots_filter ran on this handle, by the form of the sampling tail: *tiles_only the one
 * block-statistics launch (every active slot at topk <= 8 without a nucleus), *chain the four launches.  Either may be NULL. */
int pmhip_s2_slots_filter_steps(const pmhip_s2* h, int* tiles_only, int* chain);

/* EDIT REQUESTS IN A SLOTS STEP (new entries within ABI 11): pmhip_pipeline_step_slots_filter with a
 * re-masking count per slot, counts_host a HOST int32 [B] or NULL.  counts_host[b] == -1: slot b re-masks its record's num_mask,
 * as through every entry above; 0 <= counts_host[b] <= tokens: it re-masks exactly that many positions, 0 leaving its row as the
 * sampler merged it (its record's num_mask is then not read and may be anything).  That is what an edit needs: with the counts
 * of an edit schedule a given id is never re-masked and no mask id is left behind.  Idle slots are not looked at.
 * Every active slot's entry is validated in -1..tokens before anything is staged or launched (PMHIP_EINVAL, ids untouched; the
 * message names the slot).
 * counts_host NULL, or no active slot with an entry >= 0: the call runs exactly pmhip_pipeline_step_slots_filter -- the same
 * launches, the same graph key, the same captured graph.  Otherwise the counts travel in the pinned-ring entry of the records,
 * behind the nucleus masses (an idle slot's is 0), into a handle-owned device array, and the re-masking launch is
 * pmhip_remask_slots_counts or its choice form; the tower passes, the combines and the sampling tail stay as they are.  With
 * PMHIP_SLOTS_GRAPH this form has one further graph key, and as the counts are read from device memory that one graph serves
 * every set of counts. */
int pmhip_pipeline_step_slots_edit(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B,
                                   const int32_t* ctx_lens_host, const pmhip_slot* slots_host,
                                   const pmhip_slot_guide* guides_host, const float* choice_host /* [B] or NULL */,
                                   const float* neg_context /* [B,Ln,context_dim] or NULL */, int Ln,
                                   const int32_t* neg_lens_host /* [B] or NULL */, const float* top_p_host /* [B] or NULL */,
                                   const int32_t* counts_host /* [B] or NULL */, int flags, int64_t* pred_out, float* score_out,
                                   pmhip_stream stream);
/* Steps pmhip_pipeline_step_slots_edit ran on this handle with the re-masking form that takes a count per slot (the others ran
 * the step of the entry above).  The pointer may be NULL.  Every step of this entry is also counted by
 * pmhip_s2_slots_filter_steps, by the form of its sampling tail. */
int pmhip_s2_slots_edit_steps(const pmhip_s2* h, int* steps);

/* REGIONAL PROMPTS IN A SLOTS STEP (new entries within ABI 11): pmhip_pipeline_step_slots_edit with three
 * HOST arrays in front of `flags`, all NULL or none:
 *   ctx_seg_host  uint8  [B, L]     : the segment 0..31 of context row k of slot b, or 255 = padding
 *   tok_seg_host  uint32 [B, tokens]: bit s set = the token attends to the rows of segment s
 *   region_host   uint8  [B]        : 1 = slot b is regional, 0 = it is not
 * An active slot with region_host[b] == 1 runs the cross-attention of the pass WITH the context under its key sets, exactly as
 * pmhip_pipeline_sample_segments does for that image; its ctx_lens_host[b] is not used (the padding value subsumes the length).
 * An active slot with region_host[b] == 0 runs under ctx_lens_host[b] (L where ctx_lens_host is NULL), as through the entry above,
 * and its rows of the two segment arrays are not looked at.  Idle slots count as 0.  The pass without a context and the pass
 * against the negative context never see segments.  Either kind of slot computes the same bits whatever shares the batch.
 * Validated before anything is staged or launched (PMHIP_EINVAL, ids untouched), for ACTIVE slots: region_host[b] in {0, 1};
 * for a regional slot the rules of the *_segments entries -- every segment id in 0..31 or 255 (the message names the slot and
 * the row), every token allows a segment that is PRESENT in its slot (the message names the slot and the token), a context is
 * required, given or kept; every other slot keeps the length check of the entry above.
 * The arrays NULL, or no ACTIVE slot regional: the call runs exactly pmhip_pipeline_step_slots_edit -- the same launches, the
 * same graph key, the same captured graph.  Otherwise every layer's cross-attention of the pass with the context is two launches
 * of pmhip_attention_pick into the same buffer, first the per-image-length form with want = 0, then the per-query form with want
 * = 1; the arrays and the flags travel like the lengths (pinned ring entry -> copy kernel -> handle-owned device arrays), and
 * everything else of the step is unchanged.  PMHIP_SLOTS_KEEP_CONTEXT keeps the cross K/V only: every call brings its own
 * arrays, as with the lengths.  With PMHIP_SLOTS_GRAPH this form has one further graph key, and as the captured graph bakes in
 * the device arrays, not their contents, one graph per (B, L, pass set, ...) serves every mix of regional and plain slots and
 * every layout. */
int pmhip_pipeline_step_slots_regions(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B,
                                      const int32_t* ctx_lens_host, const pmhip_slot* slots_host,
                                      const pmhip_slot_guide* guides_host, const float* choice_host /* [B] or NULL */,
                                      const float* neg_context /* [B,Ln,context_dim] or NULL */, int Ln,
                                      const int32_t* neg_lens_host /* [B] or NULL */, const float* top_p_host /* [B] or NULL */,
                                      const int32_t* counts_host /* [B] or NULL */, const uint8_t* ctx_seg_host,
                                      const uint32_t* tok_seg_host, const uint8_t* region_host, int flags, int64_t* pred_out,
                                      float* score_out, pmhip_stream stream);
/* Steps pmhip_pipeline_step_slots_regions ran on this handle with the two-launch cross-attention (an active slot was regional;
 * the others ran the step of the entry above).  The pointer may be NULL. */
int pmhip_s2_slots_region_steps(const pmhip_s2* h, int* steps);

/* PROMPT WEIGHTS IN A SLOTS STEP (new entries within ABI 11): pmhip_pipeline_step_slots_regions with one more
 * HOST array in front of `flags`:
 *   ctx_w_host    f32    [B, L]     : the weight of context row k of slot b, 0 or in [2^-20, 2^20]
 * and region_host read as a KIND per slot: 0 = the slot runs under its length, 1 = under its key sets, 2 = under its key sets AND
 * its weights, exactly as pmhip_pipeline_sample_lens does for that image with ctx_seg_host, tok_seg_host and ctx_w_host (a weighted
 * slot without regions brings the one-segment layout: segment 0 below its length, 255 behind, every token mask with bit 0 set).
 * Idle slots count as 0.  The pass without a context and the pass against the negative context never see weights.  Every kind of
 * slot computes the same bits whatever shares the batch.
 * ctx_w_host NULL, or no ACTIVE slot of kind 2: the call runs exactly pmhip_pipeline_step_slots_regions -- the same validation
 * (kind 2 without the weights array is PMHIP_EINVAL), the same launches, the same graph key, the same captured graph.
 * Validated before anything is staged or launched (PMHIP_EINVAL, ids untouched), for ACTIVE slots: the kind in {0, 1, 2}; a
 * kind-2 slot follows the rules of a regional one and the weight rules of the *_weights entries -- every weight finite and 0 or in
 * [2^-20, 2^20] (the message names the slot and the row), every token allows a segment with a row of weight > 0 (the message names
 * the slot and the token); slots of kind 0 and 1 keep their checks, their rows of ctx_w_host are not looked at and are staged as 1.
 * ctx_w_host without the three arrays of the entry above is PMHIP_EINVAL.
 * The weights travel as in the *_weights entries: pinned ring entry -> copy kernel -> "ctx.w" -> pmhip_key_bias in the handle's
 * score unit -> "ctx.bias".  Every layer's cross-attention of the pass with the context is then THREE launches into the same buffer:
 * pmhip_attention_pick with the lengths and want = 0, pmhip_attention_pick with the key sets and want = 1,
 * pmhip_attention_pick_weighted with want = 2.  With PMHIP_SLOTS_GRAPH this form has one further graph key, and as the captured
 * graph bakes in the device arrays, not their contents, one graph per (B, L, pass set, ...) serves every mix of the three kinds,
 * every layout and every set of weights. */
int pmhip_pipeline_step_slots_weights(pmhip_s2* s2, int64_t* ids, const float* context, int L, int B,
                                      const int32_t* ctx_lens_host, const pmhip_slot* slots_host,
                                      const pmhip_slot_guide* guides_host, const float* choice_host /* [B] or NULL */,
                                      const float* neg_context /* [B,Ln,context_dim] or NULL */, int Ln,
                                      const int32_t* neg_lens_host /* [B] or NULL */, const float* top_p_host /* [B] or NULL */,
                                      const int32_t* counts_host /* [B] or NULL */, const uint8_t* ctx_seg_host,
                                      const uint32_t* tok_seg_host, const uint8_t* region_host, const float* ctx_w_host, int flags,
                                      int64_t* pred_out, float* score_out, pmhip_stream stream);
/* Steps pmhip_pipeline_step_slots_weights ran on this handle with the three-launch cross-attention (an active slot was of kind 2);
 * such a step is NOT counted by pmhip_s2_slots_region_steps, which keeps counting the two-launch form.  The pointer may be NULL. */
int pmhip_s2_slots_weight_steps(const pmhip_s2* h, int* steps);

/* The PMHIP_* development switches are read from the environment when a handle is CREATED and stay with it (its workspace,
 * fold decisions and captured graphs depend on them); editing the environment of a live handle does nothing.  These return
 * what a handle latched: bit 0 LayerNorm fold (PMHIP_LN_UNFOLD unset), bit 1 bf16 hi/lo stream (PMHIP_HILO != 0), bit 2 row
 * statistics from the producers (always set: its switch is gone), bit 3 centred hi plane (PMHIP_HILO_CENTER != 0), bit 4
 * PMHIP_BLOCKING_WAIT, bit 5 (pmhip_s2_switches only; process-wide) AMD_DIRECT_DISPATCH=0: PMHIP_GENERATE_GRAPH requests run
 * the eager loop; -1 for a NULL handle.  A tool that A/Bs a switch asserts the mode it believes it measures. */
int pmhip_s2_switches(const pmhip_s2* h);
int pmhip_vqgan_switches(const pmhip_vqgan* h);
/* The shared step 0 (PMHIP_GENERATE_FROM_MASK): *fills = how often this handle computed it (0 or 1), *hits = how many loops
 * sampled their step 0 from it without running a tower.  Either pointer may be NULL. */
int pmhip_s2_step0_shared(const pmhip_s2* h, int* fills, int* hits);
/* Slots steps this handle ran (both slots entries), by tower passes: *one_pass without guidance, *two_pass with at least one
 * active guided slot.  Either pointer may be NULL. */
int pmhip_s2_slots_steps(const pmhip_s2* h, int* one_pass, int* two_pass);
/* The same with the steps of THREE passes (slots guided against no context and against a negative context in one step,
 * pmhip_pipeline_step_slots_negative); *two_pass stays the steps of exactly two.  Any pointer may be NULL. */
int pmhip_s2_slots_passes(const pmhip_s2* h, int* one_pass, int* two_pass, int* three_pass);

/* REGIONAL PROMPTS (new entries within ABI 11, following the *_lens entries: nothing existing changes meaning; DESIGN.md section
 * 4u).  Different text for different parts of the picture: the context of image b is a concatenation of prompts, every row of it
 * belongs to a SEGMENT, and every token of the grid attends to a set of segments.
 *   ctx_seg_host  HOST uint8  [B, L]     : the segment 0..31 of context row k of image b, or 255 = padding
 *   tok_seg_host  HOST uint32 [B, tokens]: bit s set = the token attends to the rows of segment s
 * Row k takes part in token t's cross-attention iff ctx_seg[b,k] < 32 && (tok_seg[b,t] >> ctx_seg[b,k]) & 1; rows marked 255 never
 * reach a result, NaN included; image b computes what it computes at the same B with any other layout beside it.  Both NULL: the
 * call IS the entry it extends -- pmhip_s2_forward, pmhip_pipeline_sample_negative, pmhip_pipeline_generate_negative -- same
 * kernels, same graphs (so every narrower entry is reachable through these with neutral values, as the header promises for those).
 *   - validated before anything is launched, else PMHIP_EINVAL: both arrays or neither; every segment id in 0..31 or 255 (the
 *     message names the image and the row); every token allows at least one segment that is PRESENT in its image (the message
 *     names the image and the token); segments without a context are refused, and so are segments beside ctx_lens_host -- the
 *     padding value subsumes the length
 *   - they travel like the lengths: pinned ring -> copy kernel -> a handle-owned device array, from where the ONE launch that
 *     changes, the cross-attention of the pass with the context, reads them (pmhip_attention_segments).  Self-attention launches,
 *     the pass without a context of a guided step and a negative context's pass never see segments
 *   - captured graphs bake in that array, not its contents: one graph per (B, L) serves every layout of regions, under a key of
 *     its own beside the unmasked and the per-image graphs
 * The other arguments are those of the entry each extends. */
/* The handle's graph cache (new entry within ABI 11): *entries = the keys it holds -- one per (entry family, B, L, kernel forms,
 * ...) that was asked for with a graph flag --, *captured = how many of them hold captured graphs.  A test asserts with it that a
 * second layout of regions, lengths or scales replays the graph of the first.  Either pointer may be NULL. */
int pmhip_s2_graph_count(const pmhip_s2* h, int* entries, int* captured);
int pmhip_s2_forward_segments(pmhip_s2* h, const float* tokens, const float* context, int L, int B, const uint8_t* ctx_seg_host,
                              const uint32_t* tok_seg_host, float* logits_out, pmhip_stream stream);
int pmhip_pipeline_sample_segments(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                   const int32_t* ctx_lens_host, int topk, float temperature, int num_mask, const float* noise,
                                   uint64_t seed, uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                   float* score_out, int guided, float guidance_scale, float choice_t, const float* choice_noise,
                                   float top_p, const float* neg_context, int Ln, const int32_t* neg_lens_host,
                                   const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host, pmhip_stream stream);
int pmhip_pipeline_generate_segments(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                     const int32_t* ctx_lens_host, int T, const float* temps_host, const int* nmask_host,
                                     const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                     float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                     pmhip_stream copy_stream, int guided, float guidance_scale, const float* ctemps_host,
                                     float top_p, const float* neg_context, int Ln, const int32_t* neg_lens_host,
                                     const float* gscales_host, const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host);

/* PROMPT WEIGHTS (new entries within ABI 11, following the *_segments entries: nothing existing changes meaning; DESIGN.md section
 * 4w).  Emphasis: how much a context row counts.
 *   ctx_w_host  HOST f32 [B, L]: the weight w >= 0 of context row k of image b
 * Over the rows a token's segments allow, p[t,k] = w[k] exp(s[t,k]) / sum_j w[j] exp(s[t,j]); w == 1 is the unweighted row, an integer
 * n the row appearing n times, and w == 0 a row marked 255: it never reaches a result, NaN included.  NULL: the call IS the
 * *_segments entry -- same kernels, same graphs.
 *   - weights stand beside the two segment arrays, beside ctx_lens_host (where the entry has one), or alone.  Without segment arrays
 *     the engine stages neutral ones: segment 0 for the rows below the image's length, 255 behind, every token mask all ones.
 *     Weights beside explicit segments AND ctx_lens_host stay refused, as for segments
 *   - validated before anything is launched, else PMHIP_EINVAL: every weight finite and either 0 or in [2^-20, 2^20] (the message
 *     names the image and the row) -- outside that a weight is no emphasis any more, inside it log w stays clear of denormals and
 *     20 octaves on a score overflow nothing the exact path's running maximum does not already handle --; a context present; every
 *     token allows at least one row with w > 0 (the message names the image and the token)
 *   - they travel like the segments: pinned ring -> copy kernel -> pmhip_key_bias -> a handle-owned device array, from where the ONE
 *     launch that changes, the cross-attention of the pass with the context, reads them (pmhip_attention_weighted).  The pass
 *     without a context of a guided step and a negative context's pass never see weights
 *   - captured graphs bake in that array, not its contents: one graph per (B, L) serves every set of weights (and every layout of
 *     regions beside them), under one further key of the handle's graph cache (pmhip_s2_graph_count)
 * The other arguments are those of the entry each extends. */
int pmhip_s2_forward_weights(pmhip_s2* h, const float* tokens, const float* context, int L, int B, const uint8_t* ctx_seg_host,
                             const uint32_t* tok_seg_host, const float* ctx_w_host, float* logits_out, pmhip_stream stream);
/* pmhip_s2_forward_weights / _lens with the cross-attention maps of chosen layers beside the logits (new entry within ABI 11, nothing
 * existing changes meaning).  layer_bits: bit l set = layer l is chosen.  maps_out DEVICE f32 [B, tokens, L]:
 * (1 / n) * the sum over the n chosen layers of that layer's head-mean probabilities (pmhip_attention_maps on the layer's scaled Q,
 * its cached K and the call's lengths, key sets and key biases, issued directly behind the layer's cross-attention launch; the first
 * chosen layer writes, the later ones accumulate, each with scale = 1 / n).  Rows of the context that take part in no softmax are 0.
 *   - validation happens before anything is launched: the checks of pmhip_s2_forward_weights and _lens with the combination rules
 *     of pmhip_pipeline_sample_weights (the weights beside the lengths, beside the segment arrays, or alone), plus: a context is
 *     required, layer_bits != 0, no bit at or above depth, maps_out != NULL
 *   - logits_out gets, bit for bit, the logits of the matching existing entry on the same arguments
 *   - eager only: the entry adds no key to the handle's graph cache, and it clears the tap before it returns, on the error paths too:
 *     a later call of any entry runs exactly what it ran before */
int pmhip_s2_forward_maps(pmhip_s2* h, const float* tokens, const float* context, int L, int B, const int32_t* ctx_lens_host,
                          const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host, const float* ctx_w_host, uint64_t layer_bits,
                          float* logits_out, float* maps_out, pmhip_stream stream);
/* Prompt-to-prompt: ONE eager forward over B PAIRS of images (new entry within ABI 11, nothing existing changes meaning; DESIGN.md
 * section 4za).  tokens [2B * tokens, embed_dim], context [2B, L, D], logits_out [2B * tokens, n_embed]: images [0, B) carry the
 * source prompts, images [B, 2B) the edited ones.  ctx_lens_host [2B] or NULL.
 *   cross_bits  bit l set: in layer l the cross-attention of the source half is the ordinary launch on its B images, and the edited
 *               half runs pmhip_attention_control with Qs / Ks the source half's scaled Q and cached K, under
 *               row_map_host int32 [B, L] (the source row of every edited row, negative: none), blend_host f32 [B, L] and
 *               gain_host f32 [B, L] -- one row per pair
 *   self_bits   bit l set (may be 0): in layer l the edited half's FIRST self-attention runs pmhip_attention_dh on the source half's Q
 *               and K and its own V^T (self-attention injection; pointer arithmetic, no kernel of its own)
 *   - validation happens before anything is launched: the checks of pmhip_s2_forward_lens, plus: a context is required,
 *     cross_bits | self_bits != 0, no bit at or above depth, the three arrays required iff cross_bits != 0, every map entry < L, every
 *     blend in [0, 1], every gain finite and >= 0
 *   - the source half's logits are, bit for bit, those of pmhip_s2_forward_lens / pmhip_s2_forward on the source half alone
 *   - eager only: the entry adds no key to the handle's graph cache, and it clears the control before it returns, on the error paths
 *     too: a later call of any entry runs exactly what it ran before */
int pmhip_s2_forward_control(pmhip_s2* h, const float* tokens, const float* context, int L, int B, const int32_t* ctx_lens_host,
                             uint64_t cross_bits, uint64_t self_bits, const int32_t* row_map_host, const float* blend_host,
                             const float* gain_host, float* logits_out, pmhip_stream stream);
/* pmhip_s2_forward_control with the PHRASE-SCORE tap (new entry within ABI 11, nothing existing changes meaning; DESIGN.md section
 * 4zc): the arguments of pmhip_s2_forward_control, and
 *   score_bits   bit l set: layer l issues one pmhip_attention_phrase_score directly behind its cross-attention launch, on that
 *                layer's scaled Q and cached K of the two halves, under the call's lengths; with the control arrays if the layer is in
 *                cross_bits, with NULL otherwise.  scale = 1 / popcount(score_bits); the first tapped layer writes unless
 *                `accumulate` != 0, later tapped layers accumulate
 *   w_src_host, w_edit_host  f32 [B, L]: the phrase's row weights of the source and of the edited prompt, one row per pair
 *   scores       DEVICE f32 [2B, tokens], the source half in front
 *   - cross_bits | self_bits == 0 is allowed here: the logits are then those of pmhip_s2_forward_lens / pmhip_s2_forward on the 2B
 *     images, bit for bit.  In every other case they are those of pmhip_s2_forward_control on the same arguments, bit for bit
 *   - validation happens before anything is launched: the checks of pmhip_s2_forward_control (but for the one above), plus:
 *     score_bits != 0 with no bit at or above depth, the three pointers non-NULL, every weight finite and >= 0, every pair with a
 *     positive weight below its length in at least one half
 *   - the weights travel through the control staging ring, behind the control arrays
 *   - eager only: no key is added to the graph cache, and the tap is cleared with the control on every way out */
int pmhip_s2_forward_control_scores(pmhip_s2* h, const float* tokens, const float* context, int L, int B, const int32_t* ctx_lens_host,
                                    uint64_t cross_bits, uint64_t self_bits, const int32_t* row_map_host, const float* blend_host,
                                    const float* gain_host, uint64_t score_bits, const float* w_src_host, const float* w_edit_host,
                                    float* logits_out, float* scores, int accumulate, pmhip_stream stream);
int pmhip_pipeline_sample_weights(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                  const int32_t* ctx_lens_host, int topk, float temperature, int num_mask, const float* noise,
                                  uint64_t seed, uint32_t step, uint64_t image_base, float* img_out, int64_t* pred_out,
                                  float* score_out, int guided, float guidance_scale, float choice_t, const float* choice_noise,
                                  float top_p, const float* neg_context, int Ln, const int32_t* neg_lens_host,
                                  const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host, const float* ctx_w_host,
                                  pmhip_stream stream);
int pmhip_pipeline_generate_weights(pmhip_s2* s2, pmhip_vqgan* vq, int64_t* ids, const float* context, int L, int B,
                                    const int32_t* ctx_lens_host, int T, const float* temps_host, const int* nmask_host,
                                    const unsigned char* decode_host, int topk, uint64_t seed, uint64_t image_base,
                                    float* imgs_out, int use_graph, pmhip_stream stream, float* imgs_host, size_t host_stride,
                                    pmhip_stream copy_stream, int guided, float guidance_scale, const float* ctemps_host,
                                    float top_p, const float* neg_context, int Ln, const int32_t* neg_lens_host,
                                    const float* gscales_host, const uint8_t* ctx_seg_host, const uint32_t* tok_seg_host,
                                    const float* ctx_w_host);

/* Canvases beyond the token grid (new entries within ABI 11, nothing existing changes meaning): overlapping
 * model-sized windows over a larger canvas.  Both entries are gathers without atomics: two launches give the same bits.
 *
 * The canvas logits from the window logits.  win f32 [B * window_rows, V] with row stride ldw: canvas b's windows are the rows
 * [b * window_rows, (b + 1) * window_rows), window w's token `local` at w * g^2 + local.  win_u (NULL: none) a second tensor of the
 * same shape and stride with `scale` (finite): the element used is then fma(scale, c - u, u), the expression of
 * pmhip_guidance_combine, formed at load.  cover int32 [Nc, K] and weight f32 [Nc, K] on the device, 1 <= K <= 16: for canvas token
 * t the window rows that cover it.  out f32 [B * Nc, V] with row stride ldo:
 *     out[b * Nc + t] = w_0 x_0, then fma(w_k, x_k, out), k ascending over the entries with 0 <= cover[t][k] < window_rows
 *   - an entry outside [0, window_rows) is tested in front of its load and skipped: never an address, and the weight beside it is
 *     never read into a result; a window row that no entry of a canvas row names never reaches that row, NaN included; a canvas row
 *     without a valid entry is written as 0
 *   - K = 1 with weight 1 is an exact copy; row offsets are 64-bit
 *   - served: V % 4 == 0, ldw % 4 == 0, ldo % 4 == 0, both at least V, win / win_u / out 16-byte aligned; else PMHIP_EINVAL
 *   - nothing outside the [B * Nc, V] extents of out is written; the inputs are left as they are */
int pmhip_window_logits(const float* win, const float* win_u, float scale, int ldw, const int32_t* cover, const float* weight, int K,
                        int window_rows, float* out, int ldo, int B, int Nc, int V, pmhip_stream stream);
/* The canvas image from the decoded window images.  img f32 [B * ny * nx, C, S, S], canvas b's windows row-major in front of canvas
 * b + 1's; ywin int32 [Hc, 4] / yw f32 [Hc, 4]: for every canvas row up to four (window index on the y axis, weight) pairs, ascending,
 * padded with -1; xwin [Wc, 4] / xw [Wc, 4] likewise for the columns; yoff int32 [ny] / xoff int32 [nx]: the windows' offsets in
 * pixels.  out f32 [B, C, Hc, Wc], contiguous:
 *     out = sum over jy ascending (outside), jx ascending (inside) of rn(ay ax) * img[window (jy, jx)][c][y - yoff[jy]][x - xoff[jx]]
 * the first product rounded, every later one a fused multiply-add; then the clamp of pmhip_unpatchify_clamp to [-1, 1] (a NaN stays
 * a NaN).  An entry outside its axis' windows, or whose local coordinate falls outside [0, S), is tested in front of the load and
 * skipped.  A pixel one window covers with weight 1 is that window's pixel, bit for bit (within [-1, 1]). */
int pmhip_window_pixels(const float* img, const int32_t* ywin, const float* yw, const int32_t* xwin, const float* xw, const int32_t* yoff,
                        const int32_t* xoff, float* out, int B, int C, int S, int ny, int nx, int Hc, int Wc, pmhip_stream stream);

/* Per-kernel timing hook used by bench.py: when enabled, every kernel launch of the named family
 * is bracketed by hipEvents on its own stream and accumulated (count, total ms). */
int pmhip_timing_enable(int on);
int pmhip_timing_reset(void);
/* family: "gemm" (all GEMM launches = the sum of "gemm_plain", "gemm_heads", "gemm_swiglu", "gemm_resid", "gemm_resid2b": bias-only /
 * head-split q|k|v / SwiGLU w12 / residual producers on the one-workgroup kernels / on the two-workgroups-per-CU kernel),
 * "attention", "layernorm", "sample", "vq", "rowops"; returns PMHIP_EINVAL if unknown.  The accumulators are process-wide and
 * guarded by a mutex; while timing is on pmhip_pipeline_generate runs eagerly (no graph replay) and runs the tower of EVERY
 * step (no shared step 0, see PMHIP_GENERATE_FROM_MASK). */
int pmhip_timing_get(const char* family, int* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* PMHIP_H */
