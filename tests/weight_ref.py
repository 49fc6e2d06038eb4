"""The float64 restatement of PROMPT WEIGHTS (include/pmhip.h, pmhip_attention_weighted), shared by
tests/test_weights_cpu.py, tests/test_gpu_attention_weights.py and tests/test_gpu_weights.py.

The contract.  On top of the segments of tests/region_ref.py every context row k of image b carries a weight w[b, k] >= 0, and over
the keys a query's segments allow

    p[q, k] = w[k] exp(s[q, k]) / sum_j w[j] exp(s[q, j])

so an integer weight n is the row appearing n times, w == 1 is the row as without weights, and w == 0 is padding: the row reaches no
result whatever it holds, NaN included.

Written for clarity, not speed, and sharing no code with the package (nor with region_ref): loops over images and queries, float64
numpy, the weights multiplied into the exponentials -- no logarithm of a weight is formed for the result.

The score error (``score_error``), derived from the arithmetic of the kernels, not tuned.  The kernels add bias = log(w), in the
score's unit, to the score and then run the softmax of the segmented form.  Against attention_probes.score_error this adds:

  (a) the running maximum the accumulators start from is a maximum over s + bias, so |m| <= max_j |s_j + bias_j| takes the place of
      max_j |s_j| in that term (72 * 2^-23 * (max_j sum_d |q_d| |k_jd| + |m|), unchanged otherwise);
  (b) the conversion (pmhip_key_bias): log2f is the device library's, documented at 1 ulp, and ulp(x) <= 2^-23 |x|, so the bias in
      octaves is off by at most 2^-23 |bias|.  In nats mode it is multiplied by float32(ln 2): the constant is rounded (relative
      2^-24) and so is the product (relative 2^-24), together one more 2^-23 |bias|.  w == 1 gives exactly 0 and adds nothing;
  (c) ONE f32 addition (s - m) + bias per score: relative 2^-24 of a sum that lies in [-(max - min), 0] of s + bias, at most
      2 max_j |s_j + bias_j| in magnitude: 2^-23 max_j |s_j + bias_j|.

Per query row, in the kernel's unit:  2^-23 * (c max_j |bias_j| + max_j |s_j + bias_j|), c = 1 for octaves and 2 for nats, over the
keys that can reach the row; times ln 2 in exp2 mode to give nats, like the rest of the term.
"""
import numpy as np

EPS = 2.0 ** -23
LN2 = float(np.log(2.0))
PAD = 255
W_MIN, W_MAX = 2.0 ** -20, 2.0 ** 20


def allowed(key_seg, query_mask, w):
    """-> bool [B, Nq, Nkv]: key k takes part in query q's softmax iff its segment is in 0..31, the bit is set, and w[b, k] > 0"""
    ks = np.asarray(key_seg).astype(np.int64) & 0xFF
    qm = np.asarray(query_mask).astype(np.int64) & 0xFFFFFFFF
    w = np.asarray(w, np.float64)
    B, Nkv = ks.shape
    out = np.zeros((B, qm.shape[1], Nkv), bool)
    for b in range(B):
        for k in range(Nkv):
            if ks[b, k] < 32 and w[b, k] > 0:
                out[b, :, k] = ((qm[b] >> ks[b, k]) & 1) == 1
    return out


def attention(q, k, v, key_seg, query_mask, w, exp2):
    """q [B, H, Nq, dh], k / v [B, H, Nkv, dh] (what the kernel sees), key_seg [B, Nkv], query_mask [B, Nq], w [B, Nkv] ->
    float64 (ref [B, H, Nq, dh], A = sum_j p_ij |v_je|, s [B, H, Nq, Nkv]): the triple of region_ref.attention under the weights.
    s is the score the softmax runs over, q.k + log(w) in the kernel's unit (octaves when exp2), -inf where the key does not
    take part.  Rows of k / v that take part in no query of their image are never read."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    w = np.asarray(w, np.float64)
    assert np.all((w == 0) | ((w >= W_MIN) & (w <= W_MAX))), "weights are 0 or in [2^-20, 2^20]"
    ok = allowed(key_seg, query_mask, w)
    assert ok.any(-1).all(), "every query must allow at least one key with a weight above 0"
    B, H, Nq, dh = q.shape
    Nkv = k.shape[2]
    ref, A = np.zeros((B, H, Nq, dh)), np.zeros((B, H, Nq, dh))
    s = np.full((B, H, Nq, Nkv), -np.inf)
    for b in range(B):
        for h in range(H):
            for i in range(Nq):
                js = np.flatnonzero(ok[b, i])
                sc = k[b, h, js] @ q[b, h, i]                         # the kernel's unit
                nat = sc * LN2 if exp2 else sc
                e = w[b, js] * np.exp(nat - nat.max())
                p = e / e.sum()
                ref[b, h, i] = p @ v[b, h, js]
                A[b, h, i] = p @ np.abs(v[b, h, js])
                s[b, h, i, js] = sc + (np.log2(w[b, js]) if exp2 else np.log(w[b, js]))
    return ref, A, s


def score_error(q, k, s, w, exp2):
    """e_s per query row [B, H, Nq], in nats: attention_probes.score_error with (a), plus (b) and (c) of the module docstring.
    q, k: the arrays with the rows that reach no result zeroed; s: the effective scores of ``attention`` (-inf where a key does not
    take part); w [B, Nkv]."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    fin = np.isfinite(s)
    s_abs = np.where(fin, np.abs(np.where(fin, s, 0.0)), 0.0).max(-1)                       # max_j |s_j + bias_j|
    w = np.asarray(w, np.float64)
    bias = np.where(w > 0, np.log2(np.where(w > 0, w, 1.0)) * (1.0 if exp2 else LN2), 0.0)     # [B, Nkv], the kernel's unit
    b_abs = np.where(fin, np.abs(bias)[:, None, None, :], 0.0).max(-1)                      # over the keys that reach the row
    mag = (np.abs(q) @ np.swapaxes(np.abs(k), -1, -2)).max(-1) + s_abs                      # (a)
    unit = LN2 if exp2 else 1.0
    return (72.0 * EPS * mag + EPS * ((1.0 if exp2 else 2.0) * b_abs + s_abs)) * unit       # + (b) + (c)


def bias_error(w, exp2):
    """|pmhip_key_bias(w) - log(w)| allowed per element, (b) of the module docstring; 0 where w is 0 or 1 (exact there)"""
    w = np.asarray(w, np.float64)
    live = (w > 0) & (w != 1)
    exact = np.where(live, np.log2(np.where(live, w, 2.0)) * (1.0 if exp2 else LN2), 0.0)
    return np.where(live, (1.0 if exp2 else 2.0) * EPS * np.abs(exact), 0.0)


def cross_attention(attn, x, context, key_seg, query_mask, w):
    """``CrossAttention`` (weights read from the module, nothing else) on x [B, N, D] and context [B, L, Dc] in float64 under the
    segments and the weights -> float64 numpy [B, N, D] (to_out included, no residual)"""
    f = lambda t: t.detach().double().numpy()
    B, N, _ = x.shape
    h, d = attn.heads, attn.dim_head
    dead = ((np.asarray(key_seg).astype(np.int64) & 0xFF) == PAD) | (np.asarray(w) == 0)
    c = np.where(dead[:, :, None], 0.0, f(context))
    split = lambda t, n: t.reshape(B, n, h, d).transpose(0, 2, 1, 3)
    q = split(f(x) @ f(attn.to_q.weight).T * (d ** -0.5), N)
    k = split(c @ f(attn.to_k.weight).T, c.shape[1])
    v = split(c @ f(attn.to_v.weight).T, c.shape[1])
    ref, _, _ = attention(q, k, v, key_seg, query_mask, w, exp2=False)
    o = ref.transpose(0, 2, 1, 3).reshape(B, N, h * d)
    return o @ f(attn.to_out[0].weight).T + f(attn.to_out[0].bias)


# ------------------------------------------------------------------------------------------------ the operator tests' data
# (shared by the CPU test that proves the inputs bite and the GPU test that runs them)

NKVS = (1, 63, 64, 65, 129, 416)
ALL = 0xFFFFFFFF
S_FIRST, S_LAST, S_MID, S_EVEN, S_ODD, S_LOUD = 1, 2, 3, 4, 5, 6
WEIGHTS = np.array([0.0, 0.125, 1.0, 8.0], np.float32)


def layouts(nkv, nq, seed=0):
    """The three layouts of tests/test_gpu_attention_segments.py, rebuilt here (image 0: a query allowed only the first key, one
    allowed only the LAST; image 1: keys alternating between two segments, a middle tile of its own, queries allowing one, the other
    or both; image 2: text, a loud segment no query allows, and padding at random), and over them weights drawn from {0, 1/8, 1, 8}.
    Keys that a query depends on alone keep a weight above 0.  -> (key_seg uint8 [3, nkv], query_mask uint32 [3, nq], w f32 [3, nkv])"""
    rng = np.random.default_rng([seed, nkv, 4])
    ks = np.zeros((3, nkv), np.uint8)
    qm = np.full((3, nq), ALL, np.uint32)
    ks[0, nkv - 1] = S_LAST
    ks[0, 0] = S_FIRST
    qm[0, 5] = 1 << S_FIRST
    qm[0, 70 % nq] = 1 << (S_LAST if nkv > 1 else S_FIRST)
    j = np.arange(nkv)
    ks[1] = np.where(j % 2 == 0, S_EVEN, S_ODD)
    if nkv > 128:
        ks[1, 64:128] = S_MID
    i = np.arange(nq)
    qm[1] = np.where(i % 3 == 0, ALL, np.where(i % 3 == 1, (1 << S_EVEN) | (1 << S_MID), (1 << S_ODD) | (1 << S_MID)))
    qm[1, 16:32] = (1 << S_EVEN) | (1 << S_ODD)
    ks[2] = rng.choice(np.array([0, S_LOUD, PAD], np.uint8), size=nkv)
    ks[2, 0] = 0
    qm[2] = ALL & ~(1 << S_LOUD)
    w = rng.choice(WEIGHTS, size=(3, nkv)).astype(np.float32)
    live = rng.choice(WEIGHTS[1:], size=(3, nkv)).astype(np.float32)
    for b, k in [(0, 0), (0, nkv - 1), (1, 0), (1, min(1, nkv - 1)), (2, 0)]:
        w[b, k] = live[b, k]
    ok = allowed(ks, qm, w)
    qm[~ok.any(-1)] = ALL                                             # (only at the smallest key counts)
    qm[2] &= ~np.uint32(1 << S_LOUD)
    assert allowed(ks, qm, w).any(-1).all()
    return ks, qm, w


def inputs(gauss, nkv, dh=64, batch=3, heads=2, nq=80):
    """`gauss` = attention_probes.gauss.  Its data at sigma 4 under the layouts, image b using layout b % 3; image-2 layouts get
    positive queries and K rows of 512 on the loud keys; padding keys AND keys of weight 0 carry NaN in K and V.
    -> dict(q, k, v: what the kernels see; kz, vz: the same with the rows that reach no result zeroed; ks, qm, w)"""
    d = gauss((batch, heads), nq, nkv, 4.0, dh)
    ks3, qm3, w3 = layouts(nkv, nq)
    sel = np.arange(batch) % 3
    ks, qm, w = ks3[sel], qm3[sel], w3[sel]
    q, k, v = d["q"].copy(), d["k"].copy(), d["v"].copy()
    kz, vz = k.copy(), v.copy()
    for b in range(batch):
        loud = (ks[b] == S_LOUD) if b % 3 == 2 else np.zeros(nkv, bool)
        dead = (ks[b] == PAD) | (w[b] == 0)
        if b % 3 == 2:
            q[b] = np.abs(q[b])
            k[b][:, loud] = 512.0
        k[b][:, dead] = np.nan
        v[b][:, dead] = np.nan
        kz[b][:, loud | dead] = 0.0
        vz[b][:, dead] = 0.0
    return dict(q=q, k=k, v=v, kz=kz, vz=vz, ks=ks, qm=qm, w=w)


def bounds(P, d, kind, exp2):
    """`P` = attention_probes.  -> (ref, Bd, s): the reference under the weights and attention_probes.bound with the extended score
    error, taken over the rows that can reach a result"""
    nkv = d["k"].shape[-2]
    ref, A, s = attention(d["q"], d["kz"], d["vz"], d["ks"], d["qm"], d["w"], exp2)
    e_s = score_error(d["q"], d["kz"], s, d["w"], exp2)
    return ref, P.bound(kind, ref, A, e_s, nkv), s
