"""Probes for pmhip_attention_maps: a float64 reference, an element-wise bound derived from the arithmetic
(not tuned), the four forms' layouts, an exact input family, and a float32 numpy restatement of the kernels' arithmetic that can be
made wrong on purpose.  No GPU and no torch in here: tests/test_attention_maps_cpu.py proves on the CPU that the bound rejects the
faults at the very inputs tests/test_gpu_attention_maps.py runs, which holds the kernels to the same bound.

The quantity.  maps[b, q, k] = scale / heads * sum_h p_h[q, k], p_h the softmax of head h over the keys that take part in query q:
key k < n_b (the image's length), its segment allowed by the query's mask, its weight above 0; p = w exp(s) / sum w exp(s).

The bound, per element, for one launch with scale 1 (times |scale| otherwise):

    B = mean_h[(gamma + 2 e_s,h) p_h] + (heads + 2) 2^-23 ref          gamma = (Nkv + 72) 2^-23

gamma covers the Nkv-term sum of the denominator, the exponentials, the rescales of the running sum and the division, exactly as
in attention_probes.bound('f32'); a score error e moves p by a factor exp(+-e) in numerator and denominator (2 e_s p), e_s from
attention_probes.score_error over the scores the softmax runs on; the sum over the heads is heads - 1 additions and the factor
scale / heads one rounded constant and one multiplication (heads + 2 roundings of a value that is at most ref).  Under `accumulate`
one more addition rounds the stored sum: + 2^-23 |out|.  P stays f32 in bf16 mode, so one bound serves both dtypes.
"""
import numpy as np

import attention_probes as P

EPS = 2.0 ** -23
LN2 = float(np.log(2.0))
PAD = 255
NKVS = (1, 33, 77, 129, 416)
FORMS = ("plain", "lens", "segments", "weighted")
WEIGHTS = np.array([0.0, 0.125, 1.0, 8.0, 1.3], np.float32)
FAULTS = ("drop_last_key", "shift_keys", "next_query_row", "skip_head", "heads_minus_one", "swap_images")
FORM_FAULTS = {"weighted": "ignore_weight", "lens": "include_first_pad_key", "segments": "include_denied_segment"}


def layout(form, B, nq, nkv, seed=0):
    """-> dict(lens int32 [B] | None, ks uint8 [B, nkv] | None, qm uint32 [B, nq] | None, w f32 [B, nkv] | None)
    lens      {Nkv, 1, Nkv, ...}
    segments  keys cycle through three segments, every fifth key (never key 0) is padding (255); query i allows segment 0 and
              segment i % 3: segment 0, key 0, is allowed to every query
    weighted  the segments, and weights drawn from {0, 1/8, 1, 8, 1.3}; key 0 keeps 1.3"""
    out = dict(lens=None, ks=None, qm=None, w=None)
    if form == "lens":
        out["lens"] = np.array([nkv if b % 2 == 0 else 1 for b in range(B)], np.int32)
    if form in ("segments", "weighted"):
        j, i = np.arange(nkv), np.arange(nq, dtype=np.uint32)
        ks = (j % 3).astype(np.uint8)
        ks[(j % 5 == 4)] = PAD
        out["ks"] = np.tile(ks, (B, 1))
        for b in range(B):                                        # the images differ: image b pads key 5 b + 2 as well
            if 5 * b + 2 < nkv:
                out["ks"][b, 5 * b + 2] = PAD
        out["qm"] = np.tile((np.uint32(1) | (np.uint32(1) << (i % 3))).astype(np.uint32), (B, 1))
    if form == "weighted":
        w = np.random.default_rng([seed, nkv, 11]).choice(WEIGHTS, size=(B, nkv)).astype(np.float32)
        w[:, 0] = 1.3
        out["w"] = w
    return out


def allowed(lay, B, nq, nkv):
    """bool [B, nq, nkv]: key k takes part in query q's softmax"""
    ok = np.ones((B, nq, nkv), bool)
    if lay["lens"] is not None:
        n = np.clip(lay["lens"], 1, nkv)
        ok &= (np.arange(nkv)[None, :] < n[:, None])[:, None, :]
    if lay["ks"] is not None:
        ks = lay["ks"].astype(np.int64)[:, None, :]
        ok &= (ks < 32) & (((lay["qm"].astype(np.int64)[:, :, None] >> np.minimum(ks, 31)) & 1) == 1)
    if lay["w"] is not None:
        ok &= (lay["w"] > 0)[:, None, :]
    return ok


def poison(k, ok, nkv_pad):
    """K [B, H, nkv, dh] -> [B, H, nkv_pad, dh] with NaN in every row that takes part in no query of its image and in [nkv, nkv_pad)"""
    B, H, nkv, dh = k.shape
    kp = np.full((B, H, nkv_pad, dh), np.nan, np.float32)
    kp[:, :, :nkv] = k
    dead = ~ok.any(1)                                             # [B, nkv]
    for b in range(B):
        kp[b][:, :nkv][:, dead[b]] = np.nan
    return kp


def reference(q, k, ok, w, exp2):
    """float64: (ref [B, Nq, Nkv] at scale 1, p [B, H, Nq, Nkv], s_eff [B, H, Nq, Nkv]: the scores the softmax runs on, in the
    kernel's unit, -inf where the key does not take part).  Rows of k that take part nowhere are never read."""
    q, k = np.asarray(q, np.float64), np.nan_to_num(np.asarray(k, np.float64))
    s = q @ np.swapaxes(k, -1, -2)
    if w is not None:
        w = np.asarray(w, np.float64)
        s = s + np.where(w > 0, np.log2(np.where(w > 0, w, 1.0)) * (1.0 if exp2 else LN2), 0.0)[:, None, None, :]
    s = np.where(ok[:, None], s, -np.inf)
    nat = s * LN2 if exp2 else s
    e = np.exp(nat - nat.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    return p.mean(1), p, s


def bound(q, k, ref, p, s, exp2, scale=1.0, accumulate_out=None):
    """the module docstring's B, element-wise [B, Nq, Nkv]"""
    nkv = s.shape[-1]
    kz = np.nan_to_num(np.asarray(k, np.float64))
    e_s = P.score_error(q, kz, np.where(np.isfinite(s), s, 0.0), exp2)                      # [B, H, Nq]
    gamma = (nkv + 72) * EPS
    heads = p.shape[1]
    b = ((gamma + 2 * e_s)[..., None] * p).mean(1) + (heads + 2) * EPS * ref
    b = b * abs(scale)
    if accumulate_out is not None:
        b = b + EPS * np.abs(np.asarray(accumulate_out, np.float64))
    return b


def worst(out, ref, Bd):
    """max over elements of err / B (0 / 0 = 0; a non-finite out or err > 0 = B -> inf) and its index"""
    return P.worst_ratio(out, ref, Bd)


# ------------------------------------------------------------------------------------------------------------- the exact family

def exact_inputs(B, H, nq, nkv, dh, ok, seed=0):
    """q_i = 16 e_{i mod dh}; k[b, h, j, d] = 0 if j == key(b, h, d) else -16: the score of query i is 0 on key(b, h, i mod dh) and
    -256 elsewhere, an off-target probability is 0 in f32 in both units, the on-target one exactly 1, and the map is exactly
    count / heads (bit-exact for heads = 4).  key(b, h, d) is drawn from the keys EVERY query of image b allows.
    -> (q, k, expect [B, nq, nkv] float32)"""
    rng = np.random.default_rng([seed, nkv, dh, H])
    q = np.zeros((B, H, nq, dh), np.float32)
    q[:, :, np.arange(nq), np.arange(nq) % dh] = 16.0
    k = np.full((B, H, nkv, dh), -16.0, np.float32)
    expect = np.zeros((B, nq, nkv), np.float64)
    for b in range(B):
        common = np.flatnonzero(ok[b].all(0))
        assert len(common), "the layouts keep one key that every query allows"
        key = common[rng.integers(0, len(common), size=(H, dh))]
        for h in range(H):
            k[b, h, key[h], np.arange(dh)] = 0.0
            expect[b, np.arange(nq), key[h, np.arange(nq) % dh]] += 1.0
    return q, k, (expect / H).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- the emulation

def emulate(q, k, lay, exp2, scale=1.0, into=None, fault=None):
    """The kernels' arithmetic in float32 numpy: f32 scores, bias added in f32, the maximum over the keys that take part, exp in
    f32, l summed in f32, p = e * (1 / l), the heads added in order, times scale * (1 / heads), added to `into` when given.
    fault: None, one of FAULTS, a value of FORM_FAULTS, or 'accumulate_overwrites'."""
    f = np.float32
    q, k = np.asarray(q, f), np.nan_to_num(np.asarray(k, f))
    B, H, nq, dh = q.shape
    nkv = k.shape[2]
    lay = dict(lay)
    if fault == "ignore_weight":
        lay["w"] = None if lay["w"] is None else np.where(lay["w"] > 0, 1.0, 0.0).astype(f)
    if fault == "include_first_pad_key" and lay["lens"] is not None:
        lay["lens"] = np.minimum(lay["lens"] + 1, nkv)
    if fault == "include_denied_segment" and lay["qm"] is not None:
        lay["qm"] = lay["qm"] | np.uint32(2)                      # every query sees segment 1 as well
    ok = allowed(lay, B, nq, nkv)
    if fault == "drop_last_key":
        last = nkv - 1 - np.argmax(ok[..., ::-1], -1)              # each query's last key that takes part
        ok = ok.copy()
        many = ok.sum(-1) > 1
        bi, qi = np.nonzero(many)
        ok[bi, qi, last[bi, qi]] = False
    s = (q @ np.swapaxes(k, -1, -2)).astype(f)
    if lay["w"] is not None:
        w = lay["w"].astype(f)
        bias = np.where(w > 0, np.log2(np.where(w > 0, w, f(1))) * f(1.0 if exp2 else LN2), f(0)).astype(f)
        s = (s + bias[:, None, None, :]).astype(f)
    s = np.where(ok[:, None], s, f(-np.inf))
    m = s.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = (np.exp2(s - m) if exp2 else np.exp(s - m)).astype(f)
    e = np.where(ok[:, None], e, f(0))
    l = e.sum(-1, keepdims=True, dtype=f)
    p = (e * (f(1) / l)).astype(f)
    heads = list(range(H))
    if fault == "skip_head":
        heads = heads[:-1]
    acc = np.zeros((B, nq, nkv), f)
    for h in heads:
        acc = (acc + p[:, h]).astype(f)
    div = H - 1 if fault == "heads_minus_one" and H > 1 else H
    v = (acc * f(f(scale) * (f(1) / f(div)))).astype(f)
    if fault == "shift_keys":
        v = np.roll(v, 1, axis=-1)
    if fault == "next_query_row":
        i = np.arange(nq)
        v = v[:, np.minimum(i + 1, nq - 1)]
    if fault == "swap_images":
        v = v[::-1]
    if into is None or fault == "accumulate_overwrites":
        return np.where(ok, v, f(0)) if into is None else np.where(ok, v, np.asarray(into, f))
    return np.where(ok, (np.asarray(into, f) + v).astype(f), np.asarray(into, f))


def fault_applies(fault, lay, B, nq, nkv, H):
    """(with one key every map is exactly 1: rows and images cannot be told apart)"""
    return {"drop_last_key": nkv >= 2, "shift_keys": nkv >= 2, "next_query_row": nq >= 2 and nkv >= 2, "skip_head": H >= 2, "heads_minus_one": H >= 2,
            "swap_images": B >= 2 and nkv >= 2, "ignore_weight": lay["w"] is not None and nkv >= 2,
            "include_first_pad_key": lay["lens"] is not None and bool((lay["lens"] < nkv).any()),
            "include_denied_segment": lay["ks"] is not None and nkv >= 2, "accumulate_overwrites": True}[fault]


def gauss_case(form, nkv, dh, heads=3, B=2, nq=80, sigma=4.0):
    """The Gauss family (attention_probes.gauss, scores of standard deviation sigma in the kernel's unit) under `form`'s layout, NaN
    in the K rows that take part nowhere.  -> dict(q, k [B, H, nkv_pad, dh] as the kernel sees it, lay, ok)"""
    g = P.gauss((B, heads), nq, nkv, sigma, dh)
    lay = layout(form, B, nq, nkv)
    ok = allowed(lay, B, nq, nkv)
    assert ok.any(-1).all()
    return dict(q=g["q"], k=poison(g["k"], ok, -(-nkv // 64) * 64), lay=lay, ok=ok)
