"""Probes for the local blend: a float64 reference of pmhip_attention_phrase_score, an element-wise bound
derived from the arithmetic (not tuned), the test inputs, an exact input family, a float32 numpy restatement of the kernels'
arithmetic that can be made wrong on purpose, and numpy restatements of pmhip_phrase_region and pmhip_blend_tokens.  No GPU and no
torch in here: tests/test_local_blend_cpu.py proves on the CPU that the bound rejects the named faults at the very inputs
tests/test_gpu_local_blend.py runs, which holds the kernels to the same bound.

The quantity, per pair b and query q (ns, nt: the pair's clamped lengths; ps, pt, has, P: tests/control_ref.py, P = pt without control):

    score_s[q] (+)= scale / heads * sum_h sum_{k < ns} w_s[k] ps_h[q, k]
    score_t[q] (+)= scale / heads * sum_h sum_{j < nt} w_t[j] P_h[q, j]

The bound, per element, for scale 1 (times |scale| otherwise), eps = 2^-23; w_t' = (1 - blend) where has, 1 elsewhere; w_s' = blend
where has, 0 elsewhere (control_ref.weights; without control w_t' = 1, w_s' = 0, gain = 1):

    B_s = mean_h[(gamma_s + 2 e_s,h) sum_k w_s,k ps_h,k]                                               the source softmax
        + (1 + heads Ls + 2 + 3) eps ref_s                                                             product, sums, factor
    B_t = mean_h[sum_j w_t,j gain_j (w_t',j (gamma_t + 2 e_t,h) pt_h,j + w_s',j (gamma_s + 2 e_s,h) ps_h,mj)]   the two softmaxes
        + (4 + 1 + heads Lt + 2 + 3) eps ref_t                                                         blend, product, sums, factor
    under `accumulate`: + eps |out|                                                                    the one rounding of the sum

    gamma_x = (L_x + 72) eps   the L_x-term sum of a softmax's denominator, its exponentials, the rescales of the running sum and the
                               division, exactly as in control_ref / attnmap_ref.bound
    e_x                        attention_probes.score_error over the scores that softmax runs on: a score error e moves p by a factor
                               exp(+-e) in numerator and denominator (2 e p)
    4 eps                      1 - blend, its product with pt, the fused blend * ps + ..., the product with gain (control_ref); kept
                               without control too, where those operations do not run
    1 eps                      the product with the row weight
    (heads L + 2) eps          every term is >= 0, so the heads * L additions into a lane's register and the two that join the four
                               lanes of a query (MFMA kernel) err by at most eps of the final sum each
    3 eps                      the constant scale * (1 / heads): the reciprocal, the product, and the product with the sum
There is no rounding of P to bf16 in any kernel, so one bound serves both dtypes.
"""
import numpy as np

import attention_probes as P
import control_ref as C

EPS = C.EPS
SHAPES = C.SHAPES
LENS = C.LENS
FAULTS = ("weights_ignored", "weights_of_the_other_half", "map_ignored", "blend_ignored", "gain_dropped", "sum_over_heads",
          "source_length_ignored", "target_length_ignored", "pairs_swapped", "accumulate_dropped", "source_from_target_softmax")
CONTROL_FAULTS = ("map_ignored", "blend_ignored", "gain_dropped")


def row_weights(B, Ls, Lt):
    """-> (w_s [B, Ls], w_t [B, Lt]) float32: a phrase-like run of ones (from Ls // 3 in the source, from Lt // 2 in the target, an
    eighth of the context long, pair b shifted by b), 1/2 at every thirteenth source row and 2 at every eleventh target row -- some of
    them at or behind a shortened length --, 0 elsewhere; row 0 of pair 0 carries 1 so that a length of 1 leaves a weight"""
    def one(L, start, every, at, value):
        w = np.zeros((B, L), np.float32)
        k = np.arange(L)
        for b in range(B):
            lo = min(start + b, L - 1)
            w[b, lo:lo + max(1, L // 8)] = 1.0
            w[b, k % every == (at + b) % every] = value
        w[0, 0] = 1.0
        return w
    return one(Ls, Ls // 3, 13, 5, 0.5), one(Lt, Lt // 2, 11, 7, 2.0)


def case(Ls, Lt, dh, sigma, kind, H=2, B=2, nq=80, control=True):
    """control_ref.case (the Gauss family for both passes, the controls, the lengths) with the row weights beside it; control False
    drops row_map / blend / gain (P = pt)"""
    d = C.case(Ls, Lt, dh, sigma, kind, H=H, B=B, nq=nq)
    del d["v"]
    d["w_s"], d["w_t"] = row_weights(B, Ls, Lt)
    if not control:
        d["row_map"] = d["blend"] = d["gain"] = None
    return d


def poison(d):
    """-> (Ks [B, H, Ls_pad, dh], Kt [B, H, Lt_pad, dh]) with NaN in every row at or behind the pair's length, the padding included"""
    B, H, Ls, dh = d["ks"].shape
    Lt = d["kt"].shape[2]
    ns, nt = C.clamp(d["lens_s"], B, Ls), C.clamp(d["lens_t"], B, Lt)
    ksp = np.full((B, H, C.pad64(Ls), dh), np.nan, np.float32)
    ktp = np.full((B, H, C.pad64(Lt), dh), np.nan, np.float32)
    for b in range(B):
        ksp[b, :, :ns[b]] = d["ks"][b, :, :ns[b]]
        ktp[b, :, :nt[b]] = d["kt"][b, :, :nt[b]]
    return ksp, ktp


def _control_weights(d):
    """control_ref.weights, or its values without control: (has, m, w_t', w_s', gain), all [B, Lt], 0 behind nt"""
    if d["row_map"] is not None:
        return C.weights(d)
    B, Lt = d["kt"].shape[0], d["kt"].shape[2]
    live = np.arange(Lt)[None, :] < C.clamp(d["lens_t"], B, Lt)[:, None]
    z = np.zeros((B, Lt))
    return z.astype(bool), z.astype(np.int64), live * 1.0, z, live * 1.0


def reference(d, exp2):
    """float64 at scale 1 -> dict(ref_s, ref_t [B, Nq]; Ts, Tt_t, Tt_s [B, H, Nq]: per head, the weighted sum of the source softmax
    and the target / source parts of the weighted P; the scores ss, st; the lengths).  A case of the exact family carries its
    probabilities (exactly 0 or 1 in f32, not in float64) and they are taken instead."""
    B, H, nq, dh = d["qt"].shape
    Ls, Lt = d["ks"].shape[2], d["kt"].shape[2]
    ns, nt = C.clamp(d["lens_s"], B, Ls), C.clamp(d["lens_t"], B, Lt)
    ps, ss = C._softmax64(d["qs"], d["ks"], ns, exp2)
    pt, st = C._softmax64(d["qt"], d["kt"], nt, exp2)
    if "ps" in d:
        ps, pt = d["ps"], d["pt"]
    has, m, w_t, w_s, g = _control_weights(d)
    psm = np.take_along_axis(ps, np.broadcast_to(m[:, None, None, :], pt.shape), -1)                 # ps[q, m_j]
    ws, wt = d["w_s"].astype(np.float64), d["w_t"].astype(np.float64)
    live_s = np.arange(Ls)[None, :] < ns[:, None]
    Ts = (ps * (ws * live_s)[:, None, None, :]).sum(-1)
    Tt_t = (pt * (wt * g * w_t)[:, None, None, :]).sum(-1)
    Tt_s = (psm * (wt * g * w_s)[:, None, None, :]).sum(-1)
    return dict(ref_s=Ts.mean(1), ref_t=(Tt_t + Tt_s).mean(1), Ts=Ts, Tt_t=Tt_t, Tt_s=Tt_s, ss=ss, st=st, ns=ns, nt=nt)


def bound(d, r, exp2, scale=1.0, into=None):
    """the module docstring's (B_s, B_t), element-wise [B, Nq] each.  into: the pair of arrays `accumulate` adds to (the rounding of
    that sum is granted on the float64 value of what is stored)"""
    H = d["qt"].shape[1]
    Ls, Lt = d["ks"].shape[2], d["kt"].shape[2]
    live_s = (np.arange(Ls)[None, :] < r["ns"][:, None])[:, None, :, None]
    live_t = (np.arange(Lt)[None, :] < r["nt"][:, None])[:, None, :, None]
    e_s = P.score_error(d["qs"], np.where(live_s, d["ks"], 0.0), r["ss"], exp2)                      # [B, H, Nq]
    e_t = P.score_error(d["qt"], np.where(live_t, d["kt"], 0.0), r["st"], exp2)
    g_s, g_t = (Ls + 72) * EPS + 2 * e_s, (Lt + 72) * EPS + 2 * e_t
    b_s = (g_s * r["Ts"]).mean(1) + (1 + H * Ls + 2 + 3) * EPS * r["ref_s"]
    b_t = (g_t * r["Tt_t"] + g_s * r["Tt_s"]).mean(1) + (4 + 1 + H * Lt + 2 + 3) * EPS * r["ref_t"]
    b_s, b_t = b_s * abs(scale), b_t * abs(scale)
    if into is not None:
        b_s = b_s + EPS * np.abs(np.asarray(into[0], np.float64) + scale * r["ref_s"])
        b_t = b_t + EPS * np.abs(np.asarray(into[1], np.float64) + scale * r["ref_t"])
    return b_s, b_t


def expected(r, scale=1.0, into=None):
    """float64: what a launch leaves in (score_s, score_t)"""
    a, c = scale * r["ref_s"], scale * r["ref_t"]
    return (a, c) if into is None else (np.asarray(into[0], np.float64) + a, np.asarray(into[1], np.float64) + c)


def worst(out, ref, Bd):
    """over both outputs: the larger err / B and its (which, pair, query)"""
    a, ia = P.worst_ratio(out[0], ref[0], Bd[0])
    c, ic = P.worst_ratio(out[1], ref[1], Bd[1])
    return (a, ("s",) + ia) if a >= c else (c, ("t",) + ic)


def into_arrays(B, nq, seed=0):
    """what an accumulating launch finds: positive, of the scores' magnitude"""
    rng = np.random.default_rng([seed, B, nq, 17])
    return rng.uniform(0.25, 1.0, (B, nq)).astype(np.float32), rng.uniform(0.25, 1.0, (B, nq)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- the exact family

def exact_case(Ls, Lt, dh, kind, H=4, B=2, nq=80, seed=0, control=True):
    """control_ref.exact_case (every probability exactly 0 or 1, blend in {0, 1/2, 1}, gain in {1/2, 1, 2}, at most two target rows per
    source row) with weights drawn from {0, 1}: every weighted P is a multiple of 1/4, a query's sum over keys and 4 heads stays below
    32, and the score is a multiple of 1/16 -- exact in f32.  expected(reference(d, exp2)) is the expectation, the same in both units"""
    d = C.exact_case(Ls, Lt, dh, kind, H=H, B=B, nq=nq, seed=seed)
    del d["v"]
    rng = np.random.default_rng([seed, Ls, Lt, 23])
    d["w_s"] = rng.integers(0, 2, (B, Ls)).astype(np.float32)
    d["w_t"] = rng.integers(0, 2, (B, Lt)).astype(np.float32)
    if not control:
        d["row_map"] = d["blend"] = d["gain"] = None
    return d


# ------------------------------------------------------------------------------------------------------------- the emulation

def emulate(d, exp2, scale=1.0, into=None, fault=None):
    """The kernels' arithmetic in float32 numpy on the finite arrays of case(): both softmaxes, the gather, (1 - blend) pt + blend ps,
    times gain, times the row weight, summed over the keys, the heads added in order, times scale * (1 / heads), added to `into` when
    given.  -> (score_s, score_t).  fault: None or one of FAULTS --
      weights_ignored             every row below the length counts 1
      weights_of_the_other_half   score_s sums under w_t, score_t under w_s (by row index; rows the other half lacks count 0)
      map_ignored                 no key has a source               blend_ignored   a mapped key takes the source whole (blend 1)
      gain_dropped                gain 1                            sum_over_heads  the heads are summed, not averaged
      source_length_ignored       the source softmax, `has` and score_s run over all Ls rows
      target_length_ignored       the target softmax and score_t run over all Lt rows
      pairs_swapped               pair b runs under pair b ^ 1's weights and controls
      accumulate_dropped          the launch overwrites what it should add to
      source_from_target_softmax  score_s sums the TARGET pass's probabilities (by row index)"""
    assert fault is None or fault in FAULTS, fault
    f = np.float32
    B, H, nq, dh = d["qt"].shape
    Ls, Lt = d["ks"].shape[2], d["kt"].shape[2]
    ns, nt = C.clamp(d["lens_s"], B, Ls), C.clamp(d["lens_t"], B, Lt)
    ctl = d["row_map"] is not None
    ws, wt = d["w_s"].astype(f), d["w_t"].astype(f)
    if ctl:
        rm, bl, g = d["row_map"].astype(np.int64), d["blend"].astype(f), d["gain"].astype(f)
    else:
        rm, bl, g = np.full((B, Lt), -1, np.int64), np.zeros((B, Lt), f), np.ones((B, Lt), f)
    if fault == "pairs_swapped":
        idx = np.arange(B) ^ 1
        idx = np.where(idx < B, idx, np.arange(B))
        rm, bl, g, ws, wt = rm[idx], bl[idx], g[idx], ws[idx], wt[idx]
    if fault == "source_length_ignored":
        ns = np.full(B, Ls, np.int64)
    if fault == "target_length_ignored":
        nt = np.full(B, Lt, np.int64)
    if fault == "gain_dropped":
        g = np.ones_like(g)
    if fault == "weights_ignored":
        ws, wt = np.ones_like(ws), np.ones_like(wt)
    if fault == "weights_of_the_other_half":
        fit = lambda w, L: np.pad(w, ((0, 0), (0, max(0, L - w.shape[1]))))[:, :L]
        ws, wt = fit(wt, Ls), fit(ws, Lt)
    ps, pt = C._softmax32(d["qs"], d["ks"], ns, exp2), C._softmax32(d["qt"], d["kt"], nt, exp2)
    live_s = np.arange(Ls)[None, :] < ns[:, None]
    live_t = np.arange(Lt)[None, :] < nt[:, None]
    has = live_t & (rm >= 0) & (rm < ns[:, None]) & (bl != 0)
    if fault == "map_ignored":
        has = np.zeros_like(has)
    if fault == "blend_ignored":
        bl = np.where(has, f(1), bl)
    psm = np.take_along_axis(ps, np.broadcast_to(np.where(has, rm, 0)[:, None, None, :], pt.shape), -1)
    mixed = (bl[:, None, None, :] * psm + ((f(1) - bl).astype(f)[:, None, None, :] * pt).astype(f)).astype(f)
    p = (g[:, None, None, :] * np.where(has[:, None, None, :], mixed, pt)).astype(f) if ctl else pt
    p = np.where(live_t[:, None, None, :], p, f(0))
    src = ps
    if fault == "source_from_target_softmax":
        src = np.pad(pt, ((0, 0),) * 3 + ((0, max(0, Ls - Lt)),))[..., :Ls]
    term_s = (np.where(live_s, ws, f(0))[:, None, None, :] * src).astype(f).sum(-1, dtype=f)          # [B, H, Nq]
    term_t = (np.where(live_t, wt, f(0))[:, None, None, :] * p).astype(f).sum(-1, dtype=f)
    acc_s, acc_t = np.zeros((B, nq), f), np.zeros((B, nq), f)
    for h in range(H):
        acc_s, acc_t = (acc_s + term_s[:, h]).astype(f), (acc_t + term_t[:, h]).astype(f)
    factor = f(f(scale) * (f(1) if fault == "sum_over_heads" else f(1) / f(H)))
    vs, vt = (acc_s * factor).astype(f), (acc_t * factor).astype(f)
    if into is None or fault == "accumulate_dropped":
        return vs, vt
    return (np.asarray(into[0], f) + vs).astype(f), (np.asarray(into[1], f) + vt).astype(f)


def fault_applies(fault, d, into=None):
    """whether the fault changes the arithmetic at all at these inputs (with one source and one target key every probability is 1 and
    every weight of row_weights is 1; without a length array there is no length to get wrong; without control there is no map, blend
    or gain; without `into` nothing to add to)"""
    B, H = d["qt"].shape[:2]
    Ls, Lt = d["ks"].shape[2], d["kt"].shape[2]
    many = Ls >= 2 and Lt >= 2
    ctl = d["row_map"] is not None
    if fault in CONTROL_FAULTS and not ctl:
        return False
    has, m, w_t, w_s, g = _control_weights(d)
    seen = d["w_t"] > 0                                        # a key of weight 0 shows nothing of its control
    short = lambda lens, L: lens is not None and bool((C.clamp(lens, B, L) < L).any())
    return {"weights_ignored": many, "weights_of_the_other_half": many,
            "map_ignored": many and bool((has & seen & (g > 0)).any()),
            "blend_ignored": many and bool((has & seen & (g > 0) & (w_t > 0)).any()),
            "gain_dropped": bool((seen & (g != 1) & (w_t + w_s > 0)).any()),
            "sum_over_heads": H >= 2,
            "source_length_ignored": Ls >= 2 and short(d["lens_s"], Ls),
            "target_length_ignored": Lt >= 2 and short(d["lens_t"], Lt),
            "pairs_swapped": B >= 2 and many, "accumulate_dropped": into is not None, "source_from_target_softmax": many}[fault]


# ------------------------------------------------------------------------------------------------------------- region and blend

def region(score_s, score_t, g, threshold, grow):
    """pmhip_phrase_region in numpy: float32 [B, g*g] twice -> uint8 [B, g*g].  threshold * max is ONE float32 product, the compare
    is a float32 compare, the union is dilated `grow` times by a 3 x 3 maximum with clipped borders"""
    f = np.float32
    s, t = np.asarray(score_s, f), np.asarray(score_t, f)
    B = s.shape[0]
    assert s.shape == t.shape == (B, g * g)
    cut = lambda x: (f(threshold) * x.max(1, keepdims=True)).astype(f)
    m = ((s >= cut(s)) | (t >= cut(t))).reshape(B, g, g)
    for _ in range(grow):
        wide = np.pad(m, ((0, 0), (1, 1), (1, 1)))
        m = np.any([wide[:, 1 + dy:1 + dy + g, 1 + dx:1 + dx + g] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    return m.reshape(B, g * g).astype(np.uint8)


def blend(mask, pred_s, merged_s, score_s, pred_t, merged_t, score_t):
    """pmhip_blend_tokens in numpy -> the edited half's (pred, merged, score): the source half's where mask == 0"""
    keep = np.asarray(mask) != 0
    return np.where(keep, pred_t, pred_s), np.where(keep, merged_t, merged_s), np.where(keep, score_t, score_s)
