"""Case builders, numpy emulations and named faults for the operators of the two text towers (paintmind_amd/csrc/t5ops.hip,
clipops.hip, attn_wave16.h; DESIGN.md sections 4zk and 4zl).  numpy only; not a conftest, not collected.

tests/test_wave16_probes_cpu.py runs the emulations WITH a fault against the float64 restatements and bounds of tests/t5_ref.py and
tests/clip_ref.py and asserts that the cases below reject it; tests/test_gpu_wave16_probes.py launches the kernels on the SAME cases
with the same checks.  No fault is ever compiled into the library: faults exist only here.

Cases (B = 3 images, H = 3 heads, so every (image, head) stride is odd; every Q, K, V is bf16-representable, the bias table is f32):
    selector   two-hot codes: key k carries e_(k % 32) + e_(32 + k // 32), so Q[q] . K[k] is 2 g for k = t(q), g for a half match and
               0 otherwise (one-hot K[k] = e_k stops at 64 keys; the edge list goes to 77).  t differs per head and per image.
               relbias adds a table of ONE +64 entry per head, at a delta that differs per head, in three variants: `selector_qk`
               (g = 128: Q . K wins, 256 against at most 128 + 64), `selector_bias` (g = 8: the bias wins, 64 against at most 16) and
               `selector_both` (g = 128 in even query rows, 8 in odd ones: the two compete row by row).  V holds small integers that
               encode (key, image, head).  A row whose largest float64 score leads every other allowed one by >= 40 must equal the V row
               of that key BIT FOR BIT (the others weigh <= e^-40 = 4e-18 each: l rounds to 1 and the sum to V); the rule is applied to
               the float64 scores, never to a kernel's output.
    ordered    scores that depend on the key alone (`pattern`): rising, falling, spike_first, spike_last,
               spike_in_last_partial_block, huge_jumps (the first key of every 16 raises the maximum by 64), very_negative (every score
               below -1e4, spread of order 1).  Head 0 builds them as Q = 8 e_0, K[k] = (s_k / 8) e_0 (very_negative: Q = 128 e_0 + e_1,
               K[k] = -80 e_0 + t_k e_1, products of bf16-representable factors); relbias head 1 has Q = 0 and the pattern over the
               delta axis of the table, head 2 half of each.  Causal heads 1 and 2 scale the pattern by 1/2 and -1.  V random per key.
    gauss      the value_case of the kernel tests: random Q / 8, K, V (and table): `gauss`; Q scaled until max |s| reaches 500
               (relbias) or 100 (causal): `gauss_reach`.
Shapes: L in LS; L_pad = round_up(L, 4) and that + 12; relbias kv_lens in triples from `lens_sets(L)`.

emulate_relbias / emulate_causal restate the kernels in float32 at the block level, over flat copies of the operands that end in a
NaN guard, so that a wrong stride or an unclamped index reads what the kernel would read (another row, another head, or NaN past the
end).  They are judged by the same bounds as the kernels, not compared with them bit for bit.

Faults (FAULTS_BOTH, FAULTS_RELBIAS, FAULTS_CAUSAL; what each one changes is written where `_emulate` applies it):
    tail_rows_not_clamped   the query rows >= L of the last tile are columns of their own in both matrix products: left unclamped they
                            change no stored element.  The fault is therefore the tile treated as full: rows q0 + c >= L are read
                            unclamped AND stored, into the first rows of the next image (the emulation lets the stray stores land
                            last; on the GPU the order is open, which the two-launch and image-alone checks cover).
    PRECISION_FAULTS        p_truncated (bf16 mode: P truncated, not rounded, before the matrix core) and diag_p_rounded_to_bf16
                            (causal bf16: the diagonal tile's P rounded to bf16).  Rounding costs ub A, which the bound grants P;
                            truncation costs up to a whole ulp, 2 ub A, one-sided.  They are NOT in the list of faults that must be
                            rejected; the CPU file records how far each one gets (test_precision_faults_are_outside_what_the_bound_sees).
`fault_applies` says by rule where a fault cannot change anything.  DESIGNATED names the family that must reject each fault.

Row operators: emulate_rmsnorm (lane / chunk layout of rmsnorm_kernel), emulate_geglu, emulate_gelu, emulate_split_heads, each with
its faults (ROW_FAULTS) and `row_fault_applies`.
"""
import math

import numpy as np

import clip_ref as RC
import t5_ref as RT
from attention_probes import bf16_round, bf16_trunc, is_bf16  # noqa: F401  (is_bf16 is used by the tests)

F32 = np.float32
NB, NH = 3, 3
LS = (1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 77)
LOG2E = F32(1.4426950408889634)
NAN = float("nan")
EXACT_MARGIN = 40.0

FAULTS_BOTH = ("drop_last_key", "include_first_masked_key", "v_pad_not_zeroed", "k_stride_is_L", "vt_stride_is_L", "o_not_rescaled",
               "l_not_rescaled", "second_tile_dropped", "p_chunk_order", "next_query_row", "next_head", "tail_rows_not_clamped")
FAULTS_RELBIAS = ("bias_delta_negated", "bias_delta_off_by_one", "bias_row_of_next_head", "bias_centre_from_L_pad", "kv_lens_of_next_image",
                  "kv_lens_zero_not_clamped", "bias_of_clamped_key_row")
FAULTS_CAUSAL = ("diagonal_exclusive", "diagonal_from_wrong_tile", "matrix_part_sees_diagonal", "gather_halves_swapped",
                 "diag_group_read_rule")
PRECISION_FAULTS = {"relbias": ("p_truncated",), "causal": ("p_truncated", "diag_p_rounded_to_bf16")}
FAULTS = {"relbias": FAULTS_BOTH + FAULTS_RELBIAS, "causal": FAULTS_BOTH + FAULTS_CAUSAL}

PATTERNS = ("rising", "falling", "spike_first", "spike_last", "spike_in_last_partial_block", "huge_jumps", "very_negative")
FAMILIES = {"relbias": ("selector_qk", "selector_bias", "selector_both") + tuple("ordered_" + p for p in PATTERNS) + ("gauss", "gauss_reach"),
            "causal": ("selector",) + tuple("ordered_" + p for p in PATTERNS) + ("gauss", "gauss_reach")}

# the family that MUST reject each fault wherever it applies (the CPU file asserts it; the other families may reject it too)
DESIGNATED = {
    "drop_last_key": "ordered", "include_first_masked_key": "gauss", "v_pad_not_zeroed": "gauss", "k_stride_is_L": "selector",
    "vt_stride_is_L": "selector", "o_not_rescaled": "ordered", "l_not_rescaled": "ordered", "second_tile_dropped": "selector",
    "p_chunk_order": "selector", "next_query_row": "selector", "next_head": "selector", "tail_rows_not_clamped": "selector",
    "bias_delta_negated": "selector", "bias_delta_off_by_one": "selector", "bias_row_of_next_head": "selector",
    "bias_centre_from_L_pad": "selector", "kv_lens_of_next_image": "selector", "kv_lens_zero_not_clamped": "gauss",
    "bias_of_clamped_key_row": "ordered", "diagonal_exclusive": "selector", "diagonal_from_wrong_tile": "selector",
    "matrix_part_sees_diagonal": "gauss", "gather_halves_swapped": "selector", "diag_group_read_rule": "selector"}


def round_up(v, m):
    return (v + m - 1) // m * m


def pads(L):
    return (round_up(L, 4), round_up(L, 4) + 12)


def lens_sets(L):
    """kv_lens triples: every value of {1, 15, 16, 17, 31, 32, 33, L - 1, L} clipped to L, and 0 and L + 5 for the clamp"""
    vals = sorted({min(x, L) for x in (1, 15, 16, 17, 31, 32, 33, L - 1, L) if x >= 1}, reverse=True)
    seq = [0, vals[0], L + 5] + vals[1:]
    seq += [L] * (-len(seq) % NB)
    return [tuple(seq[i:i + NB]) for i in range(0, len(seq), NB)]


def clamp_len(v, L):
    return min(max(int(v), 1), L)


# ---------------------------------------------------------------------------------------------------------------------------------
# case builders
# ---------------------------------------------------------------------------------------------------------------------------------
def pattern(name, N):
    """N scores along an axis (keys, or the deltas of a table row); multiples of 1/4 with at most 8 significant bits where Q . K must
    carry them"""
    i = np.arange(N)
    base = (i % 5) * 0.25
    if name == "rising":
        return 0.5 * i
    if name == "falling":
        return -0.5 * i
    if name == "spike_first":
        return np.where(i == 0, 30.0, base)
    if name == "spike_last":
        return np.where(i == N - 1, 30.0, base)
    if name == "spike_in_last_partial_block":
        start = 16 * ((N - 1) // 16)                                        # the last 16-key tile lies inside the last 32-key block
        return np.where(i == start + (N - 1 - start) // 2, 40.0, base)
    if name == "huge_jumps":
        return 64.0 * (i // 16) - (i % 16)
    if name == "very_negative":
        return -10240.0 + ((7 * i) % 11) * 0.25 - 1.0
    raise KeyError(name)


def _codes(idx):
    """two-hot codes [..., 64] of the integers idx < 96"""
    idx = np.asarray(idx)
    c = np.zeros(idx.shape + (64,))
    np.put_along_axis(c, (idx % 32)[..., None], 1.0, -1)
    np.put_along_axis(c, (32 + idx // 32)[..., None], 1.0, -1)
    return c


def _selector_values(L):
    v = np.empty((NB, NH, L, 64))
    v[..., 0::2] = (np.arange(L) + 1)[None, None, :, None]
    v[..., 1::2] = 100.0 + (np.arange(NB)[:, None] * NH + np.arange(NH)[None, :])[:, :, None, None]
    return v


def _targets(L, causal):
    """t[b, h, q]: the key query q points at"""
    q = np.arange(L)
    if causal:                                                               # a stride walk, the mirror image (half above the diagonal), below
        maps = [(7 * q + 3) % L, L - 1 - q, q // 2]
    else:
        maps = [(7 * q + 3) % L, L - 1 - q, (5 * q + 1) % L]
    t = np.stack(maps)[None].repeat(NB, 0)
    return (t + np.arange(NB)[:, None, None]) % L                           # shifted per image


_CASES = {}


def case(kind, family, L):
    """the inputs of one case, built once and never modified: q, k, v float32 [B, H, L, 64] (bf16-representable), table float32
    [H, 2L-1] (relbias), exact (bool: rows decided by a margin >= 40 are compared bit for bit)"""
    key = (kind, family, L)
    if key in _CASES:
        return _CASES[key]
    causal = kind == "causal"
    rng = np.random.default_rng(1000 * L + sum(map(ord, kind + family)))
    table = np.zeros((NH, 2 * L - 1))
    exact = False
    if family.startswith("selector"):
        exact = True
        k = 16.0 * _codes(np.broadcast_to(np.arange(L), (NB, NH, L)))
        g = {"selector": 128.0, "selector_qk": 128.0, "selector_bias": 8.0}.get(family)
        if g is None:                                                        # selector_both: Q . K wins in even rows, the bias in odd ones
            g = np.where(np.arange(L) % 2 == 0, 128.0, 8.0)[None, None, :, None]
        q = g / 16.0 * _codes(_targets(L, causal))
        v = _selector_values(L)
        if not causal:
            for h, d in enumerate((0, min(L - 1, max(L // 3, 1)), -min(L - 1, max(L // 2, 1)))):
                table[h, d + L - 1] = 64.0
    elif family.startswith("ordered_"):
        name = family[len("ordered_"):]
        s = pattern(name, L)
        q = np.zeros((NB, NH, L, 64))
        k = np.zeros((NB, NH, L, 64))
        weights = (1.0, 0.5, -1.0) if causal else (1.0, 0.0, 0.5)            # the share of the pattern that Q . K carries, per head
        for h, wgt in enumerate(weights):
            if name == "very_negative":
                q[:, h, :, 0], q[:, h, :, 1] = 128.0 * abs(wgt), float(wgt != 0.0)
                k[:, h, :, 0], k[:, h, :, 1] = -80.0, (s + 10240.0)[None]
            else:
                q[:, h, :, 0] = 8.0 * wgt
                k[:, h, :, 0] = (s / 8.0)[None]
            if not causal:
                table[h] = (1.0 - wgt) * pattern(name, 2 * L - 1)
                if wgt == 0.0:
                    k[:, h] = bf16_round(rng.standard_normal((NB, L, 64)))  # Q = 0 there: K meets nothing
        v = bf16_round(rng.standard_normal((NB, NH, L, 64)))
    elif family in ("gauss", "gauss_reach"):
        q, k, v = (bf16_round(rng.standard_normal((NB, NH, L, 64))).astype(np.float64) for _ in range(3))
        if not causal:
            table = rng.standard_normal((NH, 2 * L - 1))
        if family == "gauss":
            q = q / 8
        else:
            s = q @ k.transpose(0, 1, 3, 2)
            s = np.tril(s) if causal else s
            q = bf16_round(q * ((100.0 if causal else 500.0) / np.abs(s).max()))
    else:
        raise KeyError(family)
    out = {"kind": kind, "family": family, "L": L, "exact": exact, "q": np.asarray(q, F32), "k": np.asarray(k, F32), "v": np.asarray(v, F32),
           "table": np.asarray(table, F32) if not causal else None}
    for name, full in (("q", q), ("k", k), ("v", v)):                        # nothing was lost on the way to float32 and bf16
        assert is_bf16(out[name]) and np.array_equal(out[name].astype(np.float64), np.asarray(full, np.float64)), (key, name)
    for x in out.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    _CASES[key] = out
    return out


def layouts(c, L_pad, lens=None, pad=NAN, images=None):
    """the kernel's operands as float32 numpy: Q [B,H,L,64], K [B,H,L_pad,64], V^T [B,H,64,L_pad].  [L, L_pad) holds `pad`, and so do
    the K rows and V^T columns behind lens[b] (clamped as the kernel clamps)"""
    sel = slice(None) if images is None else images
    q, k, v = c["q"][sel], c["k"][sel], c["v"][sel]
    nb, nh, L, _ = q.shape
    K = np.full((nb, nh, L_pad, 64), pad, F32)
    Vt = np.full((nb, nh, 64, L_pad), pad, F32)
    for b in range(nb):
        n = L if lens is None else clamp_len(lens[b], L)
        K[b, :, :n] = k[b, :, :n]
        Vt[b, :, :, :n] = v[b, :, :n].transpose(0, 2, 1)
    return np.ascontiguousarray(q), K, Vt


_REFS = {}


def reference(c, lens=None):
    """float64 -> {"f32": (ref, bound), "bf16": (ref, bound), "rows": bool [B, L, H], "expect": float64 [B, L, H, 64]}; rows marks
    the query rows whose largest score leads every other allowed one by EXACT_MARGIN (exact cases only), expect their V row"""
    key = (c["kind"], c["family"], c["L"], lens)
    if key in _REFS:
        return _REFS[key]
    q, k, v = (c[x].astype(np.float64) for x in "qkv")
    L = c["L"]
    out = {}
    for name, bf in (("f32", False), ("bf16", True)):
        out[name] = RC.attention_causal(q, k, v, bf) if c["kind"] == "causal" else RT.attention(q, k, v, c["table"], lens, bf)
    s = q @ k.transpose(0, 1, 3, 2)
    if c["kind"] == "causal":
        s = np.where(np.tril(np.ones((L, L), bool)), s, -np.inf)
    else:
        idx = np.arange(L)[None, :] - np.arange(L)[:, None] + L - 1
        s = s + c["table"].astype(np.float64)[:, idx][None]
        for b in range(NB):
            s[b, :, :, (L if lens is None else clamp_len(lens[b], L)):] = -np.inf
    top = s.argmax(-1)                                                        # [B, H, L]
    rest = np.where(np.arange(L) == top[..., None], -np.inf, s).max(-1)
    rows = (s.max(-1) - rest >= EXACT_MARGIN) & c["exact"]
    out["rows"] = rows.transpose(0, 2, 1)
    out["expect"] = np.take_along_axis(v, top[..., None], 2).transpose(0, 2, 1, 3)
    _REFS[key] = out
    return out


def worst_ratio(got, ref, bound):
    """largest |got - ref| / bound; anything not finite counts as infinite"""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    if not np.isfinite(got).all():
        return math.inf
    return float((np.abs(got - ref) / bound).max())


def exact_mismatch(got, r):
    """number of elements of the exact rows that differ from the expected V row"""
    B, L, H = r["rows"].shape
    got = np.asarray(got, np.float64).reshape(B, L, H, 64)
    return int((got[r["rows"]] != r["expect"][r["rows"]]).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# where a fault can change something
# ---------------------------------------------------------------------------------------------------------------------------------
def fault_applies(fault, kind, bf16, L, L_pad):
    """False where the fault cannot change a stored element of any case of (kind, dtype, L, L_pad), by the kernel's structure"""
    KB = 32 if bf16 else 16
    causal = kind == "causal"
    if fault in ("k_stride_is_L", "vt_stride_is_L", "bias_centre_from_L_pad"):
        return L_pad != L                                                    # the same address otherwise
    if fault in ("o_not_rescaled", "l_not_rescaled"):
        return L > KB                                                        # a second block is walked
    if fault == "second_tile_dropped":
        return bf16 and L > (32 if causal else 16)                           # causal: the tile q0 = 16 has its keys 16..31 on the diagonal
    if fault == "p_chunk_order":
        return bf16 and L > (16 if causal else 4)                            # the f32 chunk order IS the key order; keys 0..3 keep their place
    if fault == "v_pad_not_zeroed":
        return not causal or (bf16 and L > 16)                               # causal f32: every matrix-core block lies wholly below q0
    if fault == "matrix_part_sees_diagonal":
        return bf16 and L > 16
    if fault == "diagonal_from_wrong_tile":
        return bf16                                                          # one tile per block in f32
    if fault == "tail_rows_not_clamped":
        return L % 16 != 0
    if fault == "include_first_masked_key":
        return not causal or L > 1                                           # causal: row L - 1 has no key behind it
    if fault in ("next_query_row", "next_head", "bias_row_of_next_head", "bias_delta_negated", "bias_of_clamped_key_row",
                 "kv_lens_of_next_image"):
        return L > 1                                   # one row, one key (weight 1 whatever its score), one delta; every kv_lens clamps to 1
    if fault == "diag_p_rounded_to_bf16":
        return bf16
    if fault == "p_truncated":
        return bf16
    return True


# ---------------------------------------------------------------------------------------------------------------------------------
# the attention kernels, block by block
# ---------------------------------------------------------------------------------------------------------------------------------
def _guarded(a, extra):
    return np.concatenate([np.asarray(a, F32).ravel(), np.full(extra, NAN, F32)])


def _take(mem, idx):
    return mem[np.clip(idx, 0, mem.size - 1)]                                # past the end: the NaN guard


def _exp_below(x, m):
    return np.exp2(((x - m).astype(F32) * LOG2E).astype(F32)).astype(F32)


_PI_BF16 = np.array([16 * ((i % 8) // 4) + 4 * (i // 8) + i % 4 for i in range(32)])   # operand index g * 8 + e -> key of the block


def _emulate(kind, q, kp, vtp, bf16, table=None, kv_lens=None, fault=None):
    causal = kind == "causal"
    q, kp, vtp = (np.asarray(a, F32) for a in (q, kp, vtp))
    B, H, L, _ = q.shape
    Lp = kp.shape[2]
    KB = 32 if bf16 else 16
    qmem, kmem, vmem = _guarded(q, 16 * 64), _guarded(kp, 64 * 64), _guarded(vtp, 64 * 64)
    tmem = None if causal else _guarded(table, 4 * Lp + 8)
    out = np.full((B * L + 16, H * 64), NAN, F32)
    stray = []
    hh, dims, c16 = np.arange(H), np.arange(64), np.arange(16)
    kstride = L if fault == "k_stride_is_L" else Lp
    vstride = L if fault == "vt_stride_is_L" else Lp
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for b in range(B):
            bh = b * H + hh
            qbh = b * H + (hh + 1) % H if fault == "next_head" else bh
            if causal:
                n_img = L
            elif kv_lens is None:
                n_img = L
            else:
                lb = int(kv_lens[(b + 1) % B if fault == "kv_lens_of_next_image" else b])
                n_img = min(lb, L) if fault == "kv_lens_zero_not_clamped" else clamp_len(lb, L)
            for q0 in range(0, L, 16):
                rows = q0 + c16
                qc = rows if fault == "tail_rows_not_clamped" else np.minimum(rows, L - 1)
                qread = np.minimum(qc + 1, L - 1) if fault == "next_query_row" else qc
                qf = _take(qmem, ((qbh[:, None] * L + qread[None, :]) * 64)[:, :, None] + dims)           # [H, 16, 64]
                n = min(L, q0 + 16) if causal else n_img
                n_key = n                                                    # keys the scores may see, and the K row clamp
                if fault == "drop_last_key":
                    n_key = n - 1
                if fault == "include_first_masked_key" and not causal:
                    n_key = n + 1
                qsee = qc + 1 if (fault == "include_first_masked_key" and causal) else qc - 1 if fault == "diagonal_exclusive" else qc
                o = np.zeros((H, 16, 64), F32)
                m = np.full((H, 16), -np.inf, F32)
                l = np.zeros((H, 16), F32)
                p = np.zeros((H, 16, KB), F32)
                k0 = 0
                for k0 in range(0, n if causal else n_key, KB):
                    keys = k0 + np.arange(KB)
                    tile0 = k0 + 16 * (np.arange(KB) // 16)
                    kr = np.minimum(keys, (n if causal else n_key) - 1)
                    kf = _take(kmem, (bh[:, None] * kstride + kr[None, :])[:, :, None] * 64 + dims)       # [H, KB, 64]
                    acc = np.matmul(qf, kf.transpose(0, 2, 1))                                          # [H, 16, KB]
                    if causal:
                        see = (keys[None, :] <= qsee[:, None]) & (tile0 < n)[None, :] & (keys < n_key)[None, :]
                        sv = np.where(see[None], acc, -np.inf).astype(F32)
                    else:
                        bkey = np.minimum(keys, n_key - 1)[None, :]
                        if fault == "bias_of_clamped_key_row":                # the K row index of the lane (its column c), not the key
                            bkey = np.minimum(tile0[None, :] + c16[:, None], n_key - 1)
                        delta = bkey - qc[:, None]
                        delta = -delta if fault == "bias_delta_negated" else delta + 1 if fault == "bias_delta_off_by_one" else delta
                        th = (hh + 1) % H if fault == "bias_row_of_next_head" else hh
                        centre = (Lp if fault == "bias_centre_from_L_pad" else L) - 1
                        bias = _take(tmem, th[:, None, None] * (2 * L - 1) + centre + delta[None])
                        sv = np.where((keys < n_key)[None, None, :], acc + bias, -np.inf).astype(F32)
                    m_new = np.maximum(m, sv.max(-1))
                    alpha = _exp_below(m, m_new)
                    p = _exp_below(sv, m_new[..., None])
                    l = (l if fault == "l_not_rescaled" else l * alpha) + p.sum(-1, dtype=F32)
                    if fault != "o_not_rescaled":
                        o = o * alpha[..., None]
                    m = m_new
                    if causal and not k0 < q0:
                        continue
                    vlimit = (n if fault == "matrix_part_sees_diagonal" else q0) if causal else n
                    pm = (bf16_trunc(p) if fault == "p_truncated" else bf16_round(p)) if bf16 else p.copy()
                    if bf16 and fault == "second_tile_dropped":
                        pm[..., 16:] = 0.0
                    if bf16 and fault == "p_chunk_order":                     # V^T loaded key by key, P left in the chunk order
                        pm = pm[..., _PI_BF16]                              # operand i: P of key pi(i) against V^T of key i
                    vt = _take(vmem, (bh[:, None] * 64 + dims[None, :])[:, :, None] * vstride + keys)     # [H, 64, KB]
                    if fault != "v_pad_not_zeroed":
                        vt = np.where(keys < vlimit, vt, F32(0))
                    o = o + np.matmul(pm, vt.transpose(0, 2, 1))
                if causal:
                    second = bf16 and q0 > k0
                    if fault == "diagonal_from_wrong_tile" and bf16:
                        second = not second
                    pd = p[..., 16:32] if second else p[..., :16]                                       # [H, 16 queries, 16 keys]
                    if bf16 and fault == "diag_p_rounded_to_bf16":
                        pd = bf16_round(pd)
                    dk = q0 + c16
                    vd = _take(vmem, (bh[:, None] * 64 + dims[None, :])[:, :, None] * vstride + dk)       # [H, 64, 16]
                    first = q0 + 4 * (c16 // 4) + (3 if fault == "diag_group_read_rule" else 0)
                    ok = (first[None, :] <= qc[:, None]) & (dk[None, :] <= qc[:, None])                   # [query, key]
                    vsel = np.where(ok[None, :, None, :], vd[:, None, :, :], F32(0))                      # [H, 16, 64, 16]
                    for g in range(4):                                       # the lane group g owns the dims 16 dt + 4 g + r
                        mine = (dims % 16) // 4 == g
                        src = np.arange(16)
                        if fault == "gather_halves_swapped":                 # group g ^ 1 weighed with the probabilities of g ^ 2 and back
                            grp = np.arange(4)
                            grp[g ^ 1], grp[g ^ 2] = g ^ 2, g ^ 1
                            src = 4 * grp[c16 // 4] + c16 % 4
                        o[:, :, mine] += np.einsum("hcj,hcdj->hcd", pd[..., src], vsel[:, :, mine, :]).astype(F32)
                val = (o * (F32(1) / l)[..., None]).astype(F32)
                if bf16:
                    val = bf16_round(val)
                for c in range(16):
                    dst = (b * L + q0 + c, val[:, c].reshape(-1))
                    if q0 + c < L:
                        out[dst[0]] = dst[1]
                    elif fault == "tail_rows_not_clamped" and dst[0] < B * L:
                        stray.append(dst)
    for row, val in stray:
        out[row] = val
    return out[:B * L].reshape(B, L, H * 64)


def emulate_relbias(q, k, v, table, kv_lens, bf16, L_pad, fault=None):
    """q [B,H,L,64], k [B,H,L_pad,64], v = V^T [B,H,64,L_pad] as the kernel takes them (NaN padding included), table [H,2L-1], kv_lens
    None or B ints -> float32 [B, L, H*64]"""
    assert k.shape[2] == L_pad and v.shape[3] == L_pad
    return _emulate("relbias", q, k, v, bf16, table, kv_lens, fault)


def emulate_causal(q, k, v, bf16, L_pad, fault=None):
    assert k.shape[2] == L_pad and v.shape[3] == L_pad
    return _emulate("causal", q, k, v, bf16, None, None, fault)


def emulate(c, bf16, L_pad, lens=None, fault=None, pad=NAN):
    q, K, Vt = layouts(c, L_pad, lens, pad)
    if c["kind"] == "causal":
        return emulate_causal(q, K, Vt, bf16, L_pad, fault)
    return emulate_relbias(q, K, Vt, c["table"], lens, bf16, L_pad, fault)


# ---------------------------------------------------------------------------------------------------------------------------------
# row operators
# ---------------------------------------------------------------------------------------------------------------------------------
ROW_FAULTS = {"rmsnorm": ("nv4_one_too_small", "mean_over_padded_width", "eps_outside_sqrt", "weight_shifted_4", "stats_from_next_row"),
              "geglu": ("gate_and_linear_swapped", "linear_from_column_j_plus_4"),
              "gelu": ("kinds_swapped",),
              "split_heads": ("tokens_pad_stride_is_tokens", "q_scale_on_k", "head_and_dim_swapped_in_vt")}
RMSNORM_DS = (1020, 1024, 1028, 2044, 2048, 2052, 4092, 4096)
RMSNORM_MS = (4, 5)
GEGLU_SHAPES = ((1, 4), (5, 64), (5, 192))                                   # (M, F)
GELU_SHAPES = ((3, 4), (3, 260))
SPLIT_SHAPE = dict(heads=3, images=3, tokens=17, tokens_pad=20)


def rmsnorm_nv4(D):
    return 4 if D <= 1024 else 8 if D <= 2048 else 16


def row_fault_applies(fault, D=None):
    if fault == "mean_over_padded_width":
        return D != 256 * rmsnorm_nv4(D)                                     # the padded width IS the width at 1024, 2048, 4096
    return True


def rmsnorm_case(D, M):
    """rows of scale 1, 2^20, 2^-20 in turn (2^-20: x^2 is far below eps, so where eps stands matters) and one all-zero row"""
    rng = np.random.default_rng(D * 1000 + M)
    scale = np.array([1.0, 2.0 ** 20, 2.0 ** -20])[np.arange(M) % 3][:, None]
    x = (rng.standard_normal((M, D)) * scale).astype(F32)
    x[3] = 0.0
    w = (1.0 + 0.5 * rng.standard_normal(D)).astype(F32)
    return x, w, 1e-6


def emulate_rmsnorm(x, w, eps, bf16, fault=None):
    """rmsnorm_kernel: lane `lane` holds the float4 at column (i * 64 + lane) * 4 for i < NV4; columns it does not hold are neither summed
    nor written (NaN here)"""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    M, D = x.shape
    nv4 = rmsnorm_nv4(D) // (2 if fault == "nv4_one_too_small" else 1)       # one dispatch step too small: 16 -> 8 -> 4 -> 2
    width = 256 * nv4
    held = min(D, width)
    xp = np.zeros((M, width), F32)
    xp[:, :held] = x[:, :held]
    v = xp.reshape(M, nv4, 64, 4)                                            # [row, i, lane, element]
    s = np.zeros((M, 64), F32)
    for i in range(nv4):
        sq = v[:, i] * v[:, i]
        s = s + ((sq[..., 0] + sq[..., 1]) + (sq[..., 2] + sq[..., 3]))
    for step in (32, 16, 8, 4, 2, 1):                                        # the wave butterfly
        s = s + s[:, np.arange(64) ^ step]
    mean = s[:, 0] / F32(width if fault == "mean_over_padded_width" else D)
    with np.errstate(divide="ignore"):
        r = F32(1) / (np.sqrt(mean) + F32(eps)) if fault == "eps_outside_sqrt" else F32(1) / np.sqrt(mean + F32(eps))
    if fault == "stats_from_next_row":
        r = np.roll(r, -1)
    wp = np.concatenate([w, np.full(8, NAN, F32)])
    wp = wp[4:4 + D] if fault == "weight_shifted_4" else wp[:D]
    out = np.full((M, D), NAN, F32)
    out[:, :held] = wp[:held] * (x[:, :held] * r[:, None].astype(F32))
    return bf16_round(out) if bf16 else out


def geglu_case(M, F):
    rng = np.random.default_rng(F + M)
    u = (3.0 * rng.standard_normal((M, 2 * F))).astype(F32)
    u[0, :4] = (30.0, -30.0, 6.0, -6.0)
    return u


def emulate_geglu(u, F, bf16, fault=None):
    u = np.asarray(u, F32)
    M = u.shape[0]
    mem = _guarded(u, 16)
    j = np.arange(F)
    base = (np.arange(M) * u.shape[1])[:, None]
    a = _take(mem, base + j + (F if fault == "gate_and_linear_swapped" else 0))
    gl = _take(mem, base + j + (0 if fault == "gate_and_linear_swapped" else F) + (4 if fault == "linear_from_column_j_plus_4" else 0))
    with np.errstate(over="ignore", invalid="ignore"):
        z = F32(0.7978845608028654) * (a + F32(0.044715) * (a * a * a))
        out = (a / (F32(1) + np.exp(F32(-2) * z))) * gl
    return bf16_round(out.astype(F32)) if bf16 else out.astype(F32)


def gelu_case(M, F):
    rng = np.random.default_rng(F)
    u = (3.0 * rng.standard_normal((M, F))).astype(F32)
    u.reshape(-1)[:4] = (1.0, -1.0, 6.0, -6.0)
    return u


def emulate_gelu(u, kind, bf16, fault=None):
    u = np.asarray(u, F32)
    if fault == "kinds_swapped":
        kind = {"erf": "quick", "quick": "erf"}[kind]
    if kind == "erf":
        erfc = np.vectorize(math.erfc, otypes=[np.float64])(-u * F32(0.70710678118654752)).astype(F32)
        out = (F32(0.5) * u) * erfc
    else:
        with np.errstate(over="ignore"):
            out = u / (F32(1) + np.exp(F32(-1.702) * u))
    return bf16_round(out.astype(F32)) if bf16 else out.astype(F32)


def split_case(kinds):
    s = SPLIT_SHAPE
    rng = np.random.default_rng(s["tokens"] + len(kinds))
    M = s["images"] * s["tokens"]
    return (rng.standard_normal((M, len(kinds) * s["heads"] * 64)) * np.exp(3 * rng.standard_normal((M, 1)))).astype(F32)


def emulate_split_heads(u, heads, tokens, tokens_pad, kinds, q_scale, bf16, fault=None):
    """split_heads_kernel -> one array per part in the kernel's layout, Q [B,H,t,64], K [B,H,tp,64], V^T [B,H,64,tp]; what is not written
    holds NaN"""
    u = np.asarray(u, F32)
    M = u.shape[0]
    B = M // tokens
    tp = tokens if fault == "tokens_pad_stride_is_tokens" else tokens_pad
    m = np.arange(M)[:, None]
    b, t = m // tokens, m % tokens
    hc = np.arange(heads * 64)[None, :]
    h, d = hc // 64, hc % 64
    outs = []
    for p, kind in enumerate(kinds):
        val = u[:, p * heads * 64:(p + 1) * heads * 64]
        size = B * heads * (tokens if kind == 0 else tokens_pad) * 64
        flat = np.full(size, NAN, F32)
        if kind == 0:
            flat[((b * heads + h) * tokens + t) * 64 + d] = val * F32(q_scale)
            shape = (B, heads, tokens, 64)
        elif kind == 1:
            flat[((b * heads + h) * tp + t) * 64 + d] = val * F32(q_scale) if fault == "q_scale_on_k" else val
            shape = (B, heads, tokens_pad, 64)
        else:
            row = (b * 64 + d) * heads + h if fault == "head_and_dim_swapped_in_vt" else (b * heads + h) * 64 + d
            flat[row * tp + t] = val
            shape = (B, heads, 64, tokens_pad)
        outs.append((bf16_round(flat) if bf16 else flat).reshape(shape))
    return outs
