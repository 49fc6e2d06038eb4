"""Probes for the attention kernels: a float64 reference, element-wise bounds that are derived from the arithmetic (not
tuned), three input families, and a numpy restatement of the bf16 kernel's arithmetic that can be made wrong on purpose.

No GPU and no torch in here: tests/test_attention_probes_cpu.py proves on the CPU that the bounds reject index faults of the
size of ONE key, tests/test_gpu_attention_probes.py holds the kernels to the same bounds.

Conventions.  q [..., Nq, dh], k [..., Nkv, dh], v [..., Nkv, dh], any leading (batch, head) dimensions.  q is what the kernel
sees: already scaled, already rounded to the compute type.  Scores q.k are octaves in exp2 mode (p = 2^s / sum) and nats
otherwise.  Every family's arrays are exactly representable in bf16, so the same arrays serve both dtypes.
"""
import numpy as np

U = 2.0 ** -8                      # unit roundoff of bf16 (8 significant bits, round to nearest)
EPS = 2.0 ** -23                   # per f32 operation: MFMA accumulation is not guaranteed to round to nearest
LN2 = float(np.log(2.0))

# key counts at which the bf16 kernel changes shape (half-tiles of 32, tiles of 64, 4-stage ring, fast / exact steps), with +-1
EDGE_NKV = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 161, 191, 192, 193, 255, 256, 257, 288, 320, 321, 383, 384, 416)
FAULTS = ("drop_last_key", "include_first_pad_key", "swap_v_keys", "shift_v_chunk", "next_query_row", "truncate_p")
# The faults the bounds must reject (tests/test_attention_probes_cpu.py).  truncate_p is not among them: truncation lowers every
# P by a factor 1 - d_j, 0 <= d_j < 2^-7, and l is the sum of the SAME truncated P, so the mean of d cancels in O / l and what is
# left, |d_j - mean| <= 2^-8 = u, is what the bound grants a correctly rounded P.  It stays in emulate_bf16 for the record.
INDEX_FAULTS = FAULTS[:-1]


def bf16_round(a):
    """float32 -> nearest bf16 (ties to even), returned as float32"""
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)
    return np.where(np.isfinite(a), r, np.asarray(a, np.float32))


def bf16_trunc(a):
    b = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return (b & np.uint32(0xFFFF0000)).view(np.float32)


def is_bf16(a):
    return bool(np.array_equal(bf16_round(a), np.asarray(a, np.float32)))


def reference(q, k, v, exp2):
    """float64: (ref[..., i, e], A[..., i, e] = sum_j p_ij |v_je|, the score matrix s[..., i, j] in the kernel's unit)"""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    s = q @ np.swapaxes(k, -1, -2)
    w = (s * LN2 if exp2 else s)
    w = w - w.max(-1, keepdims=True)
    p = np.exp(w)
    p /= p.sum(-1, keepdims=True)
    return p @ v, p @ np.abs(v), s


def score_error(q, k, s, exp2):
    """e_s per query row, in nats: f32 accumulation of a score (<= 64 products, started from -m, the running maximum):
    72 * 2^-23 * max_j (sum_d |q_d| |k_jd| + |m|), |m| <= max_j |s_j|."""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    mag = (np.abs(q) @ np.swapaxes(np.abs(k), -1, -2)).max(-1) + np.abs(s).max(-1)
    return 72.0 * EPS * mag * (LN2 if exp2 else 1.0)


def bound(kind, ref, A, e_s, nkv):
    """Element-wise absolute bound on |out - ref| for one kernel form.  ref, A [..., Nq, dh]; e_s [..., Nq].

    'bf16'     MFMA kernel (attention_bf16.hip): P is rounded to bf16 (u A in the numerator), l is the sum of the same rounded
               P (u |ref|), one output rounding (u |ref|); a score error e moves p by a factor exp(e) in numerator and
               denominator (2 e_s A):   B = 2u |ref| + (u + 2 e_s) A
    'f32'      fp32-verify kernel and the f32 dim-head kernel: gamma = (Nkv + 72) 2^-23 for the Nkv-term sums of numerator
               and denominator, the exponentials, the rescales and the division:   B = gamma (|ref| + A) + 2 e_s A
    'bf16_dh'  bf16 dim-head kernel: P stays in f32, one output rounding:   B = B_f32 + u |ref|
    """
    ref, A = np.abs(np.asarray(ref, np.float64)), np.asarray(A, np.float64)
    e = np.asarray(e_s, np.float64)[..., None]
    if kind == "bf16":
        return 2 * U * ref + (U + 2 * e) * A
    gamma = (nkv + 72) * EPS
    b = gamma * (ref + A) + 2 * e * A
    if kind == "f32":
        return b
    if kind == "bf16_dh":
        return b + U * ref
    raise ValueError(kind)


def out_layout(x):
    """[B, H, Nq, dh] -> the kernels' output layout [B * Nq, H * dh]"""
    B, H, Nq, dh = x.shape
    return np.ascontiguousarray(np.swapaxes(x, 1, 2)).reshape(B * Nq, H * dh)


def from_out_layout(o, B, H, Nq, dh):
    return np.swapaxes(np.asarray(o).reshape(B, Nq, H, dh), 1, 2)


def worst_ratio(out, ref, B):
    """max over elements of err / B (0 / 0 = 0, anything non-finite or err > 0 = B -> inf) and its index"""
    err = np.abs(np.asarray(out, np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / B)
    ratio = np.where(np.isfinite(np.asarray(out, np.float64)), ratio, np.inf)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[idx]), tuple(int(i) for i in idx)


def check_bound(out, ref, B, s, what=""):
    """-> (err / B maximum, None) or (maximum, message naming the worst (batch, head, query, column), that row's largest-weight
    key and the ratio).  out, ref, B [..., Nq, dh]; s [..., Nq, Nkv]."""
    ratio, idx = worst_ratio(out, ref, B)
    if ratio <= 1.0:
        return ratio, None
    key = int(np.argmax(s[idx[:-1]]))
    o = np.asarray(out, np.float64)[idx]
    return ratio, (f"{what}: |out - ref| exceeds the bound at (batch, head, query, column) = {idx}: out {o!r} ref {ref[idx]!r} "
                   f"bound {B[idx]!r} err / B = {ratio:.3g}; the row's largest-weight key is {key} of {s.shape[-1]}")


# ---------------------------------------------------------------------------------------------------------------- families

def selector_values(bh, j, d):
    """v[bh, j, d]: 512 distinct dyadic values +-(1 + m / 128) 2^e, m < 128, e in {0, 1} (8 significant bits, magnitudes in
    [1, 4)), that differ between neighbouring keys, columns, heads and between keys 8, 32, 64 and 256 apart."""
    code = (37 * np.asarray(j, np.int64) + 11 * np.asarray(d, np.int64) + 53 * np.asarray(bh, np.int64)) % 512
    mag = (1.0 + (code & 127) / 128.0) * (1 + ((code >> 7) & 1))
    return np.where(code >> 8, -mag, mag).astype(np.float32)


def selector_scale(exp2):
    """c in q_i = c * code: 0.75 octaves per agreeing position in exp2 mode, 0.625 nats otherwise.  The target then scores 48
    octaves / 40 nats (57.7 octaves) and stands at most c * (dh - max_{j < 32} G) above the best of the first 32 keys.  (With 1
    octave the second condition needs an agreement of +6 among the first 32 keys and fails in about one row of fifty thousand:
    the edge walk has more; with 0.75 nats it needs +10 and fails in a few rows of a hundred.)"""
    return 0.75 if exp2 else 0.625


def selector_conditions(codes, c, exp2):
    """From the code book's Gram matrix, over every target key t (the scores of its query are c * G[t, :]):
    -> (largest off-target mass sum_{j != t} base^(c (G[t, j] - dh)), largest log2 sum_j base^(c (G[t, j] - max_{j < 32} G[t, j])))"""
    codes = np.asarray(codes, np.float64)
    G = codes @ np.swapaxes(codes, -1, -2)
    n = G.shape[-1]
    lb = c if exp2 else c / LN2                              # octaves per unit of G
    off = np.exp2(lb * (G - codes.shape[-1]))
    off[..., np.arange(n), np.arange(n)] = 0.0
    mass = off.sum(-1)
    pre = G[..., :, :min(32, n)].max(-1, keepdims=True)
    log2_l = np.log2(np.exp2(lb * (G - pre)).sum(-1))
    return float(mass.max()), float(log2_l.max())


def selector(lead, nkv, exp2, dh=64, seed=0, shared_codes=False, nq=None):
    """K rows are random +-1 codes, q_i = c * code[target_i]; with nq = nkv (default) target is a permutation per (batch, head),
    so every key is the target of exactly one query; otherwise target_i = perm[i % nkv].  v = selector_values.
    -> dict(q, k, v, target, codes, c, expect): expect[..., i, :] = v[..., target_i, :]."""
    rng = np.random.default_rng([seed, nkv, dh, int(exp2)])
    lead = tuple(lead)
    nq = nkv if nq is None else nq
    nbh = int(np.prod(lead, dtype=np.int64))
    codes = rng.integers(0, 2, size=((1,) if shared_codes else (nbh,)) + (nkv, dh)).astype(np.float32) * 2 - 1
    perm = np.argsort(rng.random((nbh, nkv)), axis=-1)
    target = perm[:, np.arange(nq) % nkv]
    c = selector_scale(exp2)
    bh = np.arange(nbh)
    k = np.broadcast_to(codes, (nbh, nkv, dh))
    q = (c * k[bh[:, None], target]).astype(np.float32)
    v = selector_values(bh[:, None, None], np.arange(nkv)[None, :, None], np.arange(dh)[None, None, :])
    expect = v[bh[:, None], target]
    sh = lambda x: np.ascontiguousarray(x).reshape(lead + x.shape[1:])
    return dict(q=sh(q), k=sh(k), v=sh(v), target=sh(target), codes=codes, c=c, expect=sh(expect))


def uniform(lead, nq, nkv, dh=64):
    """Q = 0: every probability is exactly 1 and l = Nkv.  v[j, d] = 1 if j % dh == d: out[d] = count_d / Nkv, and one key
    more or less moves a column by 1 / count_d."""
    lead = tuple(lead)
    q = np.zeros(lead + (nq, dh), np.float32)
    k = bf16_round(np.random.default_rng([7, nkv, dh]).standard_normal(lead + (nkv, dh)).astype(np.float32))
    v = np.zeros(lead + (nkv, dh), np.float32)
    v[..., np.arange(nkv), np.arange(nkv) % dh] = 1.0
    return dict(q=q, k=k, v=v)


def gauss(lead, nq, nkv, sigma, dh=64, seed=0):
    """The fuzz test's data (independent normal q, k, v, rounded to bf16) with q scaled so that the scores have standard
    deviation `sigma` (in the kernel's unit)."""
    rng = np.random.default_rng([seed, nq, nkv, dh, int(sigma * 16)])
    lead = tuple(lead)
    q = bf16_round(rng.standard_normal(lead + (nq, dh)).astype(np.float32) * np.float32(sigma / np.sqrt(dh)))
    k = bf16_round(rng.standard_normal(lead + (nkv, dh)).astype(np.float32))
    v = bf16_round(rng.standard_normal(lead + (nkv, dh)).astype(np.float32))
    return dict(q=q, k=k, v=v)


def pad_kv(k, v, nkv_pad, fill=np.nan):
    """-> (K [..., nkv_pad, dh], V^T [..., dh, nkv_pad]) with `fill` in the K rows and V^T columns [Nkv, nkv_pad)"""
    nkv, dh = k.shape[-2:]
    kp = np.full(k.shape[:-2] + (nkv_pad, dh), fill, np.float32)
    kp[..., :nkv, :] = k
    vtp = np.full(v.shape[:-2] + (dh, nkv_pad), fill, np.float32)
    vtp[..., :, :nkv] = np.swapaxes(v, -1, -2)
    return kp, vtp


# ---------------------------------------------------------------------------------------------------------------- emulation

def fault_applies(fault, nq, nkv, nkv_pad=None):
    nkv_pad = -(-nkv // 64) * 64 if nkv_pad is None else nkv_pad
    return {"drop_last_key": nkv >= 2, "include_first_pad_key": nkv < nkv_pad, "swap_v_keys": nkv >= 2, "shift_v_chunk": nkv >= 16,
            "next_query_row": nq >= 2, "truncate_p": nkv >= 64}[fault]


def emulate_bf16(q, k, v, exp2, fault=None):
    """The bf16 MFMA kernel's arithmetic in numpy: f32 scores, the reference maximum taken from the first 32 keys, P = exp(s - m)
    rounded to bf16, l summed from the ROUNDED P, O = P V accumulated wide, one rounding of O / l to bf16.

    fault: None, or one of FAULTS --
      drop_last_key          the last valid key is masked as if it were padding
      include_first_pad_key  key Nkv (finite garbage in the padding) is taken as valid
      swap_v_keys            V rows j and j ^ 1 change places (both below Nkv)
      shift_v_chunk          one 8-key chunk of V^T (the last but one whole chunk) is read 8 keys late
      next_query_row         query i stores the result of query i + 1 (the last one its own)
      truncate_p             P is truncated to bf16 instead of rounded to nearest
    """
    assert fault is None or fault in FAULTS, fault
    q, k, v = (np.asarray(x, np.float32) for x in (q, k, v))
    nkv, dh = k.shape[-2:]
    if fault == "drop_last_key":
        k, v = k[..., :nkv - 1, :], v[..., :nkv - 1, :]
    elif fault == "include_first_pad_key":
        g = np.random.default_rng([99, nkv]).standard_normal((2,) + k.shape[:-2] + (1, dh)).astype(np.float32)
        k, v = np.concatenate([k, bf16_round(g[0])], -2), np.concatenate([v, bf16_round(g[1])], -2)
    elif fault == "swap_v_keys":
        j = np.arange(nkv)
        j = np.where((j ^ 1) < nkv, j ^ 1, j)
        v = v[..., j, :]
    elif fault == "shift_v_chunk":
        j = np.arange(nkv)
        c0 = 8 * (nkv // 8 - 2)
        v = v[..., np.where((j >= c0) & (j < c0 + 8), j + 8, j), :]
    s = (q @ np.swapaxes(k, -1, -2)).astype(np.float32)
    m = s[..., :32].max(-1, keepdims=True) if s.shape[-1] else np.zeros(s.shape[:-1] + (1,), np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        e = np.exp2(s - m) if exp2 else np.exp(s - m)
        p = (bf16_trunc if fault == "truncate_p" else bf16_round)(e.astype(np.float32))
        l = p.astype(np.float64).sum(-1, keepdims=True).astype(np.float32)
        o = (p.astype(np.float64) @ v.astype(np.float64)).astype(np.float32)
        out = bf16_round(o * (np.float32(1.0) / l))
    if fault == "next_query_row":
        i = np.arange(out.shape[-2])
        out = out[..., np.minimum(i + 1, len(i) - 1), :]
    return out
