"""Float64 restatements and derived element-wise bounds for the OpenCLIP text-tower operators (paintmind_amd/csrc/clipops.hip) and the
tower built from them (paintmind_amd/modules/clip_native.py).  numpy and math.erfc only; not a conftest, not
collected.

u, g(n), EPS, ub and half_ulp_bf16 are those of tests/t5_ref.py: u = 2^-24, g(n) = n u / (1 - n u), EPS = 2^-23 per operation of the
matrix core, ub = 2^-8; a bf16 OUTPUT adds half an ulp of bf16 at |y| + bound.  Nothing below is fitted to what a kernel returns.

attention_causal (attention_causal_kernel), s_qk = q . k for k <= q (Q already scaled), p = exp(s - max) / sum, out = p V: the relbias
form of tests/t5_ref.py without the bias term and with n = q + 1 keys for row q:
    e_s       72 EPS (max_k sum_d |q_d| |k_kd| + 2 max_k |s_k|), the maxima over the row's allowed keys
    f32       B = (n + 72) EPS (|ref| + A) + 2 e_s A,   A = sum_k p_k |v_k|
    bf16      B_f32 + ub A + half_ulp_bf16(|ref| + B_f32 + ub A)    (P rounded to bf16 once, in the numerator only; the diagonal tile's
              P stays f32, which the same term covers)
    The index probe (K[k] = 8 e_k, Q[q] = 8 e_t(q)): the one matching key scores 64, every other key 0.  t(q) <= q: the hit has p = 1
    exactly, every other key e^-64 = 1.6e-28, so l = 1 + q e^-64 rounds to 1 and out = V[t] + q e^-64 max|V| rounds to V[t] for any
    |V| >= 1: bit for bit.  t(q) > q: every allowed score is 0 and the row is the mean of V[0..q].

split_heads (split_heads_kernel): a copy into the layouts of pmhip_gemm_heads.  Q is ONE float32 product u * q_scale, K and V the value
    itself; bf16 rounds that float32 number to nearest even.  Exact: the restatement is numpy's float32 product (and torch's bf16 cast).

gelu kind "quick" (gelu_kernel<1>), y = x / (1 + e), e = exp(-1.702 x):
    1.702 x   the float32 constant and the product: 2 roundings, g(2) relative on the argument
    e         the argument's error scales the exponential by exp(|1.702 x| g(2)); the library exponential is within 1 ulp = 2 u
              (measured alone on an MI355X: 0.85 ulp, 1.39 u relative, tools/hwtests/erfcf_ulp.hip):  d = |1.702 x| g(2) + 2 u
    1 + e     moves by d e / (1 + e); the addition and the division                                      + 2 u (3 u granted)
    bound = (d e / (1 + e) + 3 u) |y| + |x| 2^-120 + 2^-149
    the second term is for e beyond float32 (1.702 x < -88.7: the kernel returns -0 where the exact value is below |x| e^-88.7 <
    |x| 2^-127), the third for a quotient in the subnormal range.  Beyond |1.702 x| = 200 the result is x or 0 whatever the argument's
    error, so d is capped there.

gelu kind "erf" (gelu_kernel<0>), y = 0.5 x erfc(a), a = -x sqrt(0.5), which IS 0.5 x (1 + erf(x / sqrt 2)):
    a         the float32 constant sqrt(0.5) and the product: |da| <= |a| g(2)
    erfc(a)   d ln erfc / da = -h(a), h(a) = 2 e^(-a^2) / (sqrt(pi) erfc(a)).  In closed form: a <= 0 has erfc(a) >= 1, so
              h(a) <= (2 / sqrt pi) e^(-a^2); a > 0 has erfc(a) >= (2 / sqrt pi) e^(-a^2) / (a + sqrt(a^2 + 2)) (the classical lower
              bound of the Mills ratio), so h(a) <= a + sqrt(a^2 + 2), which increases with a and is taken at |a| (1 + g(2)).
              d_arg = expm1(|a| g(2) H(a)) relative
    library   E_erfc u relative.  The ROCm installation ships no accuracy table of the device library's erfcf, so it was
              measured ALONE on an MI355X against float64 on x = -6 + i 2^-20, 12.6 million points over [-6, 6]
              (tools/hwtests/erfcf_ulp.hip): maximum 3.33 ulp, maximum relative error 3.95 u (at x = 2.346).  E_erfc = 7.9: twice the
              observed maximum, because a grid is not exhaustive.
    0.5 x     exact; the product with erfc: u (3 u granted)
    bound = (E_erfc u + d_arg + 3 u) |y| + 2^-149          where erfc(a) >= 2^-125
    bound = 0.5 |x| 2^-124                                  where erfc(a) <  2^-125 (a > 9.2, x < -13): below the normal range the
    library's relative accuracy says nothing; the exact value and whatever the library returns there both lie in [0, 2^-125].

tower: the float64 restatement of CLIPTextEmbedder.encode_with_transformer on an open_clip text tower (eval): token embedding +
    positional embedding, per block x += out_proj(causal attention of in_proj(ln_1 x)) and x += c_proj(gelu(c_fc(ln_2 x))), ln_final;
    `skip_last` blocks at the end are left out.  The tower tests compare against it with the project's fp32 contract (max abs <= 1e-3,
    DESIGN.md section 2) and, in bf16, against the stock tower in bf16 (RMS error ratio <= 1).

Worst measured |error| / bound on an MI355X over every case tests/test_gpu_clip_kernels.py launches (the figures at 1.00 are the final
bf16 rounding alone, which is attained):
    attention_causal f32 0.002 (value) 0.004 (index)   bf16 0.49 / 0.47        gelu erf f32 0.51   bf16 1.00        gelu quick f32 0.49   bf16 1.00
The f32 attention bound is slack by its 72 EPS score term; what holds the kernel's indexing there is the index probe, which is exact.
"""
import math

import numpy as np

from t5_ref import EPS, F64, U, UB, g, half_ulp_bf16, rms  # noqa: F401  (rms is re-exported for the tower tests)

E_ERFC = 7.9                 # in units of u; twice the 3.95 u measured on an MI355X (see above)
SQRT_HALF = math.sqrt(0.5)
_erfc = np.vectorize(math.erfc, otypes=[F64])          # the C library's double-precision erfc, element by element


# ---------------------------------------------------------------------------------------------------------------------------------
# causal attention
# ---------------------------------------------------------------------------------------------------------------------------------
def attention_causal(q, k, v, bf16=False):
    """q (already scaled), k, v [B, H, L, 64] (what the kernel is given, as float64) -> (ref [B, L, H*64], bound of the same shape)"""
    q, k, v = (np.asarray(a, F64) for a in (q, k, v))
    B, H, L, dh = q.shape
    allow = np.tril(np.ones((L, L), bool))
    n = np.arange(1, L + 1, dtype=F64)[:, None]
    ref = np.zeros((B, L, H * dh))
    bound = np.zeros_like(ref)
    for b in range(B):
        for h in range(H):
            s = np.where(allow, q[b, h] @ k[b, h].T, -np.inf)
            p = np.exp(s - s.max(-1, keepdims=True))
            p /= p.sum(-1, keepdims=True)
            r, A = p @ v[b, h], p @ np.abs(v[b, h])
            mag = np.where(allow, np.abs(q[b, h]) @ np.abs(k[b, h]).T, 0.0).max(-1) + 2 * np.where(allow, np.abs(s), 0.0).max(-1)
            e_s = (72.0 * EPS * mag)[:, None]
            bd = (n + 72) * EPS * (np.abs(r) + A) + 2 * e_s * A
            if bf16:
                bd = bd + UB * A
                bd = bd + half_ulp_bf16(np.abs(r) + bd)
            ref[b, :, h * dh:(h + 1) * dh] = r
            bound[b, :, h * dh:(h + 1) * dh] = bd
    return ref, bound


# ---------------------------------------------------------------------------------------------------------------------------------
# head split
# ---------------------------------------------------------------------------------------------------------------------------------
def split_heads(u, heads, tokens, nparts, q_scale, kinds):
    """u float32 [B*tokens, >= nparts*heads*64] -> one float32 array per part WITHOUT padding: kind 0 (Q) [B,H,t,64] * q_scale as one
    float32 product, kind 1 (K) [B,H,t,64], kind 2 (V) transposed [B,H,64,t]"""
    u = np.asarray(u, np.float32)
    B = u.shape[0] // tokens
    outs = []
    for p, kind in enumerate(kinds):
        part = u[:, p * heads * 64:(p + 1) * heads * 64].reshape(B, tokens, heads, 64).transpose(0, 2, 1, 3)
        if kind == 0:
            outs.append((part * np.float32(q_scale)).astype(np.float32))
        elif kind == 1:
            outs.append(part.copy())
        else:
            outs.append(part.transpose(0, 1, 3, 2).copy())
    return outs


# ---------------------------------------------------------------------------------------------------------------------------------
# the GELUs
# ---------------------------------------------------------------------------------------------------------------------------------
def gelu_erf(x):
    x = np.asarray(x, F64)
    return 0.5 * x * _erfc(-x * SQRT_HALF)


def gelu_quick(x):
    x = np.asarray(x, F64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-1.702 * x))


def gelu(x, kind):
    return {"erf": gelu_erf, "quick": gelu_quick}[kind](x)


def gelu_bound(x, kind, bf16=False):
    x = np.asarray(x, F64)
    y = np.abs(gelu(x, kind))
    if kind == "quick":
        z = 1.702 * x
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(-z)
            frac = np.where(np.isinf(e), 1.0, e / (1.0 + e))
        d = np.minimum(np.abs(z), 200.0) * g(2) + 2 * U
        b = (d * frac + 3 * U) * y + np.abs(x) * 2.0 ** -120 + 2.0 ** -149
    else:
        a = -x * SQRT_HALF
        ap = np.abs(a) * (1 + g(2))
        with np.errstate(over="ignore", under="ignore"):
            H = np.where(a > 0, ap + np.sqrt(ap * ap + 2.0), 2.0 / math.sqrt(math.pi) * np.exp(-np.minimum(a * a, 700.0)))
            d_arg = np.expm1(np.minimum(np.abs(a) * g(2) * H, 1.0))
        normal = _erfc(a) >= 2.0 ** -125
        b = np.where(normal, (E_ERFC * U + d_arg + 3 * U) * y + 2.0 ** -149, 0.5 * np.abs(x) * 2.0 ** -124)
    return b + half_ulp_bf16(y + b) if bf16 else b


# ---------------------------------------------------------------------------------------------------------------------------------
# the tower
# ---------------------------------------------------------------------------------------------------------------------------------
def layernorm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def tower(params, ids, kind, skip_last=0, eps=1e-5):
    """params: the tower's state_dict as numpy arrays (open_clip names); ids int [B, L], L = n_ctx; kind "erf" | "quick"
    -> float64 [B, L, width]"""
    P = {k: np.asarray(v, F64) for k, v in params.items()}
    ids = np.asarray(ids)
    B, L = ids.shape
    x = P["token_embedding.weight"][ids] + P["positional_embedding"]
    W = x.shape[-1]
    H = W // 64
    depth = 1 + max(int(k.split(".")[2]) for k in P if k.startswith("transformer.resblocks."))
    allow = np.tril(np.ones((L, L), bool))
    for i in range(depth - skip_last):
        pre = f"transformer.resblocks.{i}."
        h = layernorm(x, P[pre + "ln_1.weight"], P[pre + "ln_1.bias"], eps)
        qkv = h @ P[pre + "attn.in_proj_weight"].T + P[pre + "attn.in_proj_bias"]
        split = lambda t: t.reshape(B, L, H, 64).transpose(0, 2, 1, 3)                  # noqa: E731
        q, k, v = (split(qkv[..., j * W:(j + 1) * W]) for j in range(3))
        s = np.where(allow, (q * 64 ** -0.5) @ k.transpose(0, 1, 3, 2), -np.inf)
        p = np.exp(s - s.max(-1, keepdims=True))
        p /= p.sum(-1, keepdims=True)
        a = (p @ v).transpose(0, 2, 1, 3).reshape(B, L, W)
        x = x + a @ P[pre + "attn.out_proj.weight"].T + P[pre + "attn.out_proj.bias"]
        h = layernorm(x, P[pre + "ln_2.weight"], P[pre + "ln_2.bias"], eps)
        f = gelu(h @ P[pre + "mlp.c_fc.weight"].T + P[pre + "mlp.c_fc.bias"], kind)
        x = x + f @ P[pre + "mlp.c_proj.weight"].T + P[pre + "mlp.c_proj.bias"]
    return layernorm(x, P["ln_final.weight"], P["ln_final.bias"], eps)
