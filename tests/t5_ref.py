"""Float64 restatements and derived element-wise bounds for the Flan-T5 operators (paintmind_amd/csrc/t5ops.hip) and the tower built
from them (paintmind_amd/modules/t5_native.py).  numpy only; not a conftest, not collected.

u = 2^-24 (float32 round to nearest), g(n) = n u / (1 - n u) bounds the compound error of n roundings, EPS = 2^-23 per operation of
the matrix core (its accumulation is not guaranteed to round to nearest), ub = 2^-8 the unit roundoff of bf16.  A bf16 OUTPUT adds
half an ulp of bf16 at |y| + bound: 2^-9 times that magnitude rounded up to a power of two (`half_ulp_bf16`).  Nothing below is fitted
to what a kernel returns.

bucket / bias_table: T5Attention._relative_position_bucket(bidirectional=True) for delta = key - query, and the [H, 2L-1] table whose
    entry (k - q) + L - 1 is the bias of the pair (q, k).  Integer arithmetic except the logarithm, which is taken in float32 exactly
    as Hugging Face takes it (the buckets are compared EXACTLY against it in tests/test_t5_native_cpu.py).

rmsnorm (rmsnorm_kernel: one wave per row, nv = ceil(D / 256) float4 groups per lane), y = w (x r), r = 1 / sqrt(sum x^2 / D + eps):
    sum x^2   the square, two additions inside the float4, nv lane-serial additions, 6 wave levels: every term is >= 0, so the
              error is RELATIVE, g(nv + 9); the division by D and + eps: 2 more                                  nv + 11
    r         halved by the square root; the square root and the division                                       nv / 2 + 7.5
    y         x r and w (x r)                                                                                  c = nv / 2 + 9.5
    bound = g(c) |y| + 2^-149                       (contracted multiply-adds round less often)
    an all-zero row: r = 1 / sqrt(eps) is finite and y = 0 exactly.

geglu (geglu_kernel), y = x v / (1 + e), e = exp(-2 z), z = sqrt(2/pi) (x + 0.044715 x^3), which IS gelu_new(x) v
(1 + tanh z = 2 / (1 + e^(-2z))):
    z         x x, (x x) x, the float32 constant 0.044715 and its product, + x (same sign: no cancellation), the float32 constant
              sqrt(2/pi) and its product; the factor -2 is exact                                                g(7) |z|
    e         the argument's error scales the exponential by exp(2 |z| g(7)); the library exponential is within 1 ulp = 2 u
              d = 2 |z| g(7) + 2 u relative
    1 + e     moves by d e / (1 + e); the addition, the division and the product with v                           + 3 u (4 u granted)
    bound = (d e / (1 + e) + 4 u) |y| + |x v| 2^-120 + 2^-149 max(1, |v|)
    the second term is for e beyond float32 (2 z < -88.7: the kernel returns -0 v where the exact value is below |x v| e^-88.7 <
    |x v| 2^-127), the third for a quotient in the subnormal range.  Where x^3 overflows z is +-inf, e is 0 or inf, and the kernel
    returns x v or -0 v: finite, and within the bound (the exact e is then 0 or beyond float32 as well).

attention_relbias (attention_relbias_kernel), s_qk = q . k + b[(k - q) + L - 1], p = exp(s - max) / sum, out = p V:
    e_s       per query row, in nats: the float32 accumulation of a score (64 exact products of bf16-representable operands), the
              bias addition, the subtraction of the running maximum (|s - m| <= 2 max|s|) and the product with log2(e):
              e_s = 72 EPS (max_k sum_d |q_d| |k_kd| + max_k |b_k| + 2 max_k |s_k|)           (the form of tests/attention_probes.py)
              a score error e moves p by a factor exp(e) in numerator and denominator: 2 e_s A, A = sum_k p_k |v_k|
    f32       gamma = (n + 72) EPS for the n-term sums of numerator and denominator, the exponentials, the rescales by
              exp(m_old - m_new) and the division:                      B = gamma (|ref| + A) + 2 e_s A
    bf16      P is rounded to bf16 once, in the numerator only (l sums the unrounded float32 P): ub A; then the output rounding
                                                                        B = B_f32 + ub A + half_ulp_bf16(|ref| + B_f32 + ub A)
    n = the image's key count.  The index probe (Q = 0, one table entry +64): the hit key has p = 1 exactly (s - m = 0), every other
    key e^-64 = 1.6e-28, so l = 1 + (n - 1) e^-64 rounds to 1 and out = V[q + d] + (n - 1) e^-64 max|V| rounds to V[q + d] for any
    |V| >= 1: bit for bit.

tower: the float64 restatement of T5EncoderModel.forward (eval): embedding, per layer x += o(attn(rmsnorm(x))) and
    x += wo(gelu_new(wi_0 h) * wi_1 h) with h = rmsnorm(x), the final rmsnorm; block 0's bucket table serves every layer; an optional
    key count per prompt is HF's attention_mask (masked keys get weight 0).  The tower tests compare against it with the project's fp32
    contract (max abs <= 1e-3) and, in bf16, against Hugging Face's own bf16 tower (RMS error ratio <= 1).

Worst measured |error| / bound on an MI355X over every case tests/test_gpu_t5_kernels.py launches (the figures at 1.000 are the final
bf16 rounding alone, which is attained):
    rmsnorm f32 0.340   bf16 1.000        geglu f32 0.700   bf16 1.000        attention_relbias f32 0.005   bf16 0.660
The f32 attention bound is slack by its 72 EPS score term; what holds the kernel's indexing there is the index probe, which is exact.
"""
import math

import numpy as np

F64 = np.float64
U = 2.0 ** -24
EPS = 2.0 ** -23
UB = 2.0 ** -8
SQRT_2_OVER_PI = math.sqrt(2.0 / math.pi)


def g(n):
    return n * U / (1.0 - n * U)


def half_ulp_bf16(v):
    """half an ulp of bf16 at magnitude v: 2^-9 times v rounded up to a power of two (0 at 0)"""
    v = np.abs(np.asarray(v, dtype=F64))
    with np.errstate(divide="ignore"):
        e = np.ceil(np.log2(np.where(v > 0, v, 1.0)))
    return np.where(v > 0, 2.0 ** (e - 9), 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# relative-position buckets
# ---------------------------------------------------------------------------------------------------------------------------------
def bucket(delta, num_buckets=32, max_distance=128):
    """delta = key - query (int array) -> bucket, bidirectional"""
    delta = np.asarray(delta, dtype=np.int64)
    half = num_buckets // 2
    out = (delta > 0).astype(np.int64) * half
    dist = np.abs(delta)
    max_exact = half // 2
    with np.errstate(divide="ignore"):
        # float32, operation by operation, as torch evaluates log(dist.float() / max_exact) / log(max_distance / max_exact) * (half - max_exact)
        lg = np.log(dist.astype(np.float32) / np.float32(max_exact)).astype(np.float32)
        val = (lg / np.float32(math.log(max_distance / max_exact))).astype(np.float32) * np.float32(half - max_exact)
    large = max_exact + np.where(dist >= max_exact, val, 0).astype(np.int64)
    large = np.minimum(large, half - 1)
    return out + np.where(dist < max_exact, dist, large)


def bias_table(weight, L, num_buckets=32, max_distance=128):
    """weight [num_buckets, H] -> float64 [H, 2L-1]"""
    b = bucket(np.arange(-(L - 1), L), num_buckets, max_distance)
    return np.asarray(weight, F64)[b].T.copy()


# ---------------------------------------------------------------------------------------------------------------------------------
# rmsnorm
# ---------------------------------------------------------------------------------------------------------------------------------
def rmsnorm(x, w, eps):
    x, w = np.asarray(x, F64), np.asarray(w, F64)
    return w * (x / np.sqrt((x * x).mean(-1, keepdims=True) + eps))


def rmsnorm_bound(y, D, bf16=False):
    nv = -(-D // 256)
    b = g(nv / 2 + 9.5) * np.abs(y) + 2.0 ** -149
    return b + half_ulp_bf16(np.abs(y) + b) if bf16 else b


# ---------------------------------------------------------------------------------------------------------------------------------
# gated GELU
# ---------------------------------------------------------------------------------------------------------------------------------
def _z(x):
    return SQRT_2_OVER_PI * (x + 0.044715 * x ** 3)


def gelu_new(x):
    """0.5 x (1 + tanh z) written as x / (1 + e^(-2z)): the same function, without the cancellation of 1 + tanh(z) at negative z, which
    would cost the float64 REFERENCE up to 2^-53 e^(2|z|) relative (4e-6 at x = -6)"""
    x = np.asarray(x, F64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-2.0 * _z(x)))


def geglu(u, F):
    u = np.asarray(u, F64)
    return gelu_new(u[..., :F]) * u[..., F:2 * F]


def geglu_bound(u, F, bf16=False):
    u = np.asarray(u, F64)
    x, v = u[..., :F], u[..., F:2 * F]
    z = _z(x)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-2.0 * z)
        frac = np.where(np.isinf(e), 1.0, e / (1.0 + e))
        d = np.minimum(2.0 * np.abs(z), 200.0) * g(7) + 2 * U          # beyond 2|z| = 200 the result is x v or 0 whatever the argument's error
    y = np.abs(geglu(u, F))
    b = (d * frac + 4 * U) * y + np.abs(x * v) * 2.0 ** -120 + 2.0 ** -149 * np.maximum(1.0, np.abs(v))
    return b + half_ulp_bf16(y + b) if bf16 else b


# ---------------------------------------------------------------------------------------------------------------------------------
# attention with the relative-position bias
# ---------------------------------------------------------------------------------------------------------------------------------
def attention(q, k, v, table, kv_lens=None, bf16=False):
    """q, k, v [B, H, L, 64] (what the kernel is given, as float64), table [H, 2L-1], kv_lens None or [B] (clamped as the kernel clamps)
    -> (ref [B, L, H*64], bound of the same shape)"""
    q, k, v, table = (np.asarray(a, F64) for a in (q, k, v, table))
    B, H, L, dh = q.shape
    idx = np.arange(L)[None, :] - np.arange(L)[:, None] + L - 1                       # [q, k]
    ref = np.zeros((B, L, H * dh))
    bound = np.zeros_like(ref)
    for b in range(B):
        n = L if kv_lens is None else min(max(int(kv_lens[b]), 1), L)
        for h in range(H):
            bias = table[h][idx][:, :n]
            qk = q[b, h] @ k[b, h, :n].T
            s = qk + bias
            p = np.exp(s - s.max(-1, keepdims=True))
            p /= p.sum(-1, keepdims=True)
            r, A = p @ v[b, h, :n], p @ np.abs(v[b, h, :n])
            mag = (np.abs(q[b, h]) @ np.abs(k[b, h, :n]).T).max(-1) + np.abs(bias).max(-1) + 2 * np.abs(s).max(-1)
            e_s = (72.0 * EPS * mag)[:, None]
            bd = (n + 72) * EPS * (np.abs(r) + A) + 2 * e_s * A
            if bf16:
                bd = bd + UB * A
                bd = bd + half_ulp_bf16(np.abs(r) + bd)
            ref[b, :, h * dh:(h + 1) * dh] = r
            bound[b, :, h * dh:(h + 1) * dh] = bd
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------------------
# the encoder
# ---------------------------------------------------------------------------------------------------------------------------------
def encoder(params, ids, num_heads, eps=1e-6, num_buckets=32, max_distance=128, kv_lens=None):
    """params: the T5EncoderModel's state_dict as numpy arrays; ids int [B, L] -> last_hidden_state float64 [B, L, d_model]"""
    P = {k: np.asarray(v, F64) for k, v in params.items() if "block" in k or k in ("shared.weight", "encoder.final_layer_norm.weight")}
    ids = np.asarray(ids)
    B, L = ids.shape
    x = P["shared.weight"][ids]                                                         # [B, L, D]
    H = num_heads
    table = bias_table(P["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"], L, num_buckets, max_distance)
    idx = np.arange(L)[None, :] - np.arange(L)[:, None] + L - 1
    bias = table[:, idx]                                                                # [H, q, k]
    allow = np.ones((B, 1, 1, L), bool)
    if kv_lens is not None:
        n = np.clip(np.asarray(kv_lens, np.int64), 1, L)
        allow = (np.arange(L)[None, :] < n[:, None])[:, None, None, :]
    depth = 1 + max(int(k.split(".")[2]) for k in P if k.startswith("encoder.block."))
    for i in range(depth):
        pre = f"encoder.block.{i}.layer."
        h = rmsnorm(x, P[pre + "0.layer_norm.weight"], eps)
        split = lambda t: t.reshape(B, L, H, -1).transpose(0, 2, 1, 3)                  # noqa: E731
        q, k, v = (split(h @ P[pre + f"0.SelfAttention.{n_}.weight"].T) for n_ in "qkv")
        s = q @ k.transpose(0, 1, 3, 2) + bias[None]
        s = np.where(allow, s, -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        a = (p @ v).transpose(0, 2, 1, 3).reshape(B, L, -1)
        x = x + a @ P[pre + "0.SelfAttention.o.weight"].T
        h = rmsnorm(x, P[pre + "1.layer_norm.weight"], eps)
        ff = gelu_new(h @ P[pre + "1.DenseReluDense.wi_0.weight"].T) * (h @ P[pre + "1.DenseReluDense.wi_1.weight"].T)
        x = x + ff @ P[pre + "1.DenseReluDense.wo.weight"].T
    return rmsnorm(x, P["encoder.final_layer_norm.weight"], eps)


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, F64)))))
