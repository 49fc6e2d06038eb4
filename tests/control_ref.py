"""Probes for pmhip_attention_control: a float64 reference, an element-wise bound derived from the arithmetic
(not tuned), the test inputs, an exact input family, and a float32 numpy restatement of the kernels' arithmetic that can be made
wrong on purpose.  No GPU and no torch in here: tests/test_control_cpu.py proves on the CPU that the bound rejects the named faults
at the very inputs tests/test_gpu_attention_control.py runs, which holds the kernels to the same bound.

The quantity, per pair b, head h, query q (ns, nt: the pair's clamped source / target lengths):

    ps = softmax over k < ns of qs ks^T        pt = softmax over j < nt of qt kt^T        m = row_map[b, j]
    has = 0 <= m < ns and blend[b, j] != 0
    P[q, j] = gain[b, j] (has ? (1 - blend[b, j]) pt[q, j] + blend[b, j] ps[q, m] : pt[q, j])        out[q, :] = sum_j P[q, j] v[j, :]

The bound, per element e of out (eps = 2^-23; w_t = (1 - blend) where has, 1 elsewhere; w_s = blend where has, 0 elsewhere):

    B = sum_j gain_j |v_je| [ w_t,j (gamma_t + 2 e_t) pt_j  +  w_s,j (gamma_s + 2 e_s) ps_mj ]       the two softmaxes
      + (u_P + 4 eps) A                                                                              blend, gain, rounding of P
      + (Lt + 8) eps A                                                                               the accumulation of P . V
      + u_out |ref|                                                                                  the stored element

    A = sum_j P_j |v_je|
    gamma_x = (L_x + 72) eps   the L_x-term sum of a softmax's denominator, its exponentials, the rescales of the running sum and the
                               division, exactly as in attention_probes.bound('f32') and attnmap_ref.bound
    e_x                        attention_probes.score_error over the scores that softmax runs on: a score error e moves p by a factor
                               exp(+-e) in numerator and denominator (2 e p)
    4 eps                      1 - blend, its product with pt, the fused blend * ps + ..., the product with gain: one rounding each
    u_P = 2^-8                 bf16 MFMA kernel only (bf16, dim_head 64): P is rounded to bf16 for the P . V MFMA; elsewhere 0.  bf16
                               keeps 8 significant bits, so round to nearest errs by up to 2^-8 relative (attention_probes.U, the u of
                               its 'bf16' bound); with 2^-9 the correctly rounded restatement below exceeds the bound 1.84 times
    (Lt + 8) eps               Lt f32 additions into the accumulator (the MFMA's accumulation is not guaranteed to round to nearest:
                               eps, not eps / 2, per step), with 8 to spare for the products
    u_out = 2^-8               bf16 outputs only: one rounding of the result to bf16 (attention_probes.U); 0 for f32
"""
import numpy as np

import attention_probes as P

EPS = 2.0 ** -23
LN2 = float(np.log(2.0))
U_P = P.U
SHAPES = ((1, 1), (33, 17), (77, 77), (129, 77), (77, 129), (416, 231))           # (Ls, Lt)
LENS = ("full", "one_mid", "mid_full")
BLENDS = np.array([0.0, 0.5, 1.0, 0.3], np.float32)
GAINS = np.array([0.5, 1.0, 2.0, 0.0, 1.7], np.float32)
FAULTS = ("map_ignored", "map_shifted", "blend_ignored", "blend_swapped", "gain_dropped", "source_length_ignored", "target_length_off_by_one",
          "renormalised", "pairs_swapped", "next_head_source")


def pad64(n):
    return -(-n // 64) * 64


def lengths(kind, B, Ls, Lt):
    """-> (lens_s, lens_t) int32 [B] or (None, None): 'full' none given; 'one_mid' pair b: source 1 / mid, target mid / 1, alternating;
    'mid_full' source mid / full, target full / mid"""
    if kind == "full":
        return None, None
    ms, mt = max(1, (Ls + 1) // 2), max(1, (Lt + 1) // 2)
    a, c = ((1, ms), (mt, 1)) if kind == "one_mid" else ((ms, Ls), (Lt, mt))
    return (np.array([a[b % 2] for b in range(B)], np.int32), np.array([c[b % 2] for b in range(B)], np.int32))


def clamp(lens, B, L):
    return np.full(B, L, np.int64) if lens is None else np.clip(np.asarray(lens, np.int64), 1, L)


def controls(B, Ls, Lt, seed=0):
    """row_map with repeats (j and j + 1 of an even j share a row), -1 at every seventh key, entries at Ls (behind every length) at
    every eleventh, the rest spread over [0, Ls) -- so with a length below Ls some land at or behind it --, pair b shifted by b;
    blend drawn from {0, 1/2, 1, 0.3}, gain from {1/2, 1, 2, 0, 1.7}"""
    rng = np.random.default_rng([seed, Ls, Lt, 5])
    j = np.arange(Lt)
    rm = np.stack([((j // 2) * 3 + b) % Ls for b in range(B)]).astype(np.int32)
    rm[:, j % 7 == 3] = -1
    rm[:, j % 11 == 5] = Ls
    return rm, rng.choice(BLENDS, size=(B, Lt)).astype(np.float32), rng.choice(GAINS, size=(B, Lt)).astype(np.float32)


def case(Ls, Lt, dh, sigma, kind, H=2, B=2, nq=80):
    """The Gauss family (attention_probes.gauss: values exact in bf16, scores of standard deviation sigma in the kernel's unit) for both
    passes, the controls and the lengths.  Every array finite; poison() makes the kernels' view of it."""
    gs = P.gauss((B, H), nq, Ls, sigma, dh, seed=1)
    gt = P.gauss((B, H), nq, Lt, sigma, dh, seed=2)
    rm, bl, gn = controls(B, Ls, Lt)
    ls, lt = lengths(kind, B, Ls, Lt)
    return dict(qs=gs["q"], ks=gs["k"], qt=gt["q"], kt=gt["k"], v=gt["v"], row_map=rm, blend=bl, gain=gn, lens_s=ls, lens_t=lt)


def poison(d):
    """-> (Ks [B, H, Ls_pad, dh], Kt [B, H, Lt_pad, dh], V^T [B, H, dh, Lt_pad]) with NaN in every row / column at or behind the pair's
    length, the padding included: everything that may reach nothing"""
    B, H, Ls, dh = d["ks"].shape
    Lt = d["kt"].shape[2]
    ns, nt = clamp(d["lens_s"], B, Ls), clamp(d["lens_t"], B, Lt)
    ksp = np.full((B, H, pad64(Ls), dh), np.nan, np.float32)
    ktp = np.full((B, H, pad64(Lt), dh), np.nan, np.float32)
    vtp = np.full((B, H, dh, pad64(Lt)), np.nan, np.float32)
    for b in range(B):
        ksp[b, :, :ns[b]] = d["ks"][b, :, :ns[b]]
        ktp[b, :, :nt[b]] = d["kt"][b, :, :nt[b]]
        vtp[b, :, :, :nt[b]] = np.swapaxes(d["v"][b, :, :nt[b]], -1, -2)
    return ksp, ktp, vtp


def _softmax64(q, k, n, exp2):
    """float64 softmax over the first n[b] keys -> (p, s): p 0 and s 0 behind the length"""
    q, k = np.asarray(q, np.float64), np.asarray(k, np.float64)
    L = k.shape[2]
    ok = (np.arange(L)[None, :] < n[:, None])[:, None, None, :]
    s = q @ np.swapaxes(np.where(ok[..., 0, :, None], k, 0.0), -1, -2)
    nat = np.where(ok, s * LN2 if exp2 else s, -np.inf)
    e = np.exp(nat - nat.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True), np.where(ok, s, 0.0)


def weights(d):
    """-> (has bool [B, Lt] (False behind nt), m int [B, Lt] (0 where not has), w_t, w_s, gain f64 [B, Lt], all 0 behind nt)"""
    B, Lt = d["row_map"].shape
    Ls = d["ks"].shape[2]
    ns, nt = clamp(d["lens_s"], B, Ls), clamp(d["lens_t"], B, Lt)
    live = np.arange(Lt)[None, :] < nt[:, None]
    rm, bl = d["row_map"].astype(np.int64), d["blend"].astype(np.float64)
    has = live & (rm >= 0) & (rm < ns[:, None]) & (bl != 0)
    w_t = np.where(has, 1.0 - bl, 1.0) * live
    w_s = np.where(has, bl, 0.0)
    return has, np.where(has, rm, 0), w_t, w_s, d["gain"].astype(np.float64) * live


def reference(d, exp2):
    """float64 -> dict(ref [B, H, Nq, dh], A = sum_j P_j |v_j|, At / As: its target and source parts, the scores ss, st, the lengths).
    A case of the exact family carries its probabilities (exactly 0 or 1 in f32, not in float64) and they are taken instead."""
    B, H, nq, dh = d["qt"].shape
    Ls, Lt = d["ks"].shape[2], d["kt"].shape[2]
    ns, nt = clamp(d["lens_s"], B, Ls), clamp(d["lens_t"], B, Lt)
    ps, ss = _softmax64(d["qs"], d["ks"], ns, exp2)
    pt, st = _softmax64(d["qt"], d["kt"], nt, exp2)
    if "ps" in d:
        ps, pt = d["ps"], d["pt"]
    has, m, w_t, w_s, g = weights(d)
    psm = np.take_along_axis(ps, np.broadcast_to(m[:, None, None, :], pt.shape), -1)                 # ps[q, m_j]
    part_t = (g * w_t)[:, None, None, :] * pt
    part_s = (g * w_s)[:, None, None, :] * psm
    v = np.asarray(d["v"], np.float64)
    return dict(ref=(part_t + part_s) @ v, A=(part_t + part_s) @ np.abs(v), At=part_t @ np.abs(v), As=part_s @ np.abs(v), ss=ss, st=st,
                ns=ns, nt=nt)


def bound(d, r, exp2, mfma, bf16_out):
    """the module docstring's B, element-wise [B, H, Nq, dh].  mfma: the bf16 MFMA kernel (P rounded to bf16)"""
    Ls, Lt = d["ks"].shape[2], d["kt"].shape[2]
    live_s = (np.arange(Ls)[None, :] < r["ns"][:, None])[:, None, :, None]
    live_t = (np.arange(Lt)[None, :] < r["nt"][:, None])[:, None, :, None]
    e_s = P.score_error(d["qs"], np.where(live_s, d["ks"], 0.0), r["ss"], exp2)[..., None]          # [B, H, Nq, 1]
    e_t = P.score_error(d["qt"], np.where(live_t, d["kt"], 0.0), r["st"], exp2)[..., None]
    b = ((Lt + 72) * EPS + 2 * e_t) * r["At"] + ((Ls + 72) * EPS + 2 * e_s) * r["As"]                 # the two softmaxes
    b = b + ((U_P if mfma else 0.0) + 4 * EPS) * r["A"]                                               # blend, gain, rounding of P
    b = b + (Lt + 8) * EPS * r["A"]                                                                   # the accumulation
    if bf16_out:
        b = b + P.U * np.abs(r["ref"])                                                                # the stored element
    return b


def worst(out, ref, Bd):
    return P.worst_ratio(out, ref, Bd)


# ------------------------------------------------------------------------------------------------------------- the exact family

def exact_case(Ls, Lt, dh, kind, H=4, B=2, nq=80, seed=0):
    """q_i = 16 e_{i mod dh} in both passes; K = 0 on one key below the pair's length per (pair, head, dim) and -16 elsewhere: every
    probability is exactly 0 or 1 in f32, in both units.  V small integers in [-3, 3], blend in {0, 1/2, 1}, gain in {1/2, 1, 2}, and
    a map in which at most two target rows share a source row: every P is a multiple of 1/4 up to 2, every output a multiple of 1/4
    below 32 in magnitude -- exact in f32 and in bf16.  -> the dict of case() with the 0 / 1 probabilities ps, pt beside it;
    reference(d, exp2)['ref'] is the expectation, the same in both units"""
    rng = np.random.default_rng([seed, Ls, Lt, dh, H])
    q = np.zeros((B, H, nq, dh), np.float32)
    q[:, :, np.arange(nq), np.arange(nq) % dh] = 16.0
    ls, lt = lengths(kind, B, Ls, Lt)
    ns, nt = clamp(ls, B, Ls), clamp(lt, B, Lt)
    ks, kt = np.full((B, H, Ls, dh), -16.0, np.float32), np.full((B, H, Lt, dh), -16.0, np.float32)
    ps, pt = np.zeros((B, H, nq, Ls)), np.zeros((B, H, nq, Lt))
    for b in range(B):
        for h in range(H):
            key_s, key_t = rng.integers(0, ns[b], dh), rng.integers(0, nt[b], dh)
            ks[b, h, key_s, np.arange(dh)] = 0.0
            kt[b, h, key_t, np.arange(dh)] = 0.0
            ps[b, h, np.arange(nq), key_s[np.arange(nq) % dh]] = 1.0
            pt[b, h, np.arange(nq), key_t[np.arange(nq) % dh]] = 1.0
    j = np.arange(Lt)
    rm = np.stack([np.where(j % 4 == 1, j - 1, j) + b for b in range(B)]).astype(np.int32)            # (entries >= Ls: none)
    rm[:, j % 7 == 3] = -1
    return dict(qs=q, ks=ks, qt=q.copy(), kt=kt, v=rng.integers(-3, 4, (B, H, Lt, dh)).astype(np.float32), row_map=rm,
                blend=rng.choice(BLENDS[:3], size=(B, Lt)).astype(np.float32), gain=rng.choice(GAINS[:3], size=(B, Lt)).astype(np.float32),
                lens_s=ls, lens_t=lt, ps=ps, pt=pt)


# ------------------------------------------------------------------------------------------------------------- the emulation

def _softmax32(q, k, n, exp2):
    """the kernels' softmax in float32: f32 scores, the maximum over the keys below n, exp in f32, l summed in f32, p = e * (1 / l)"""
    f = np.float32
    L = k.shape[2]
    ok = (np.arange(L)[None, :] < n[:, None])[:, None, None, :]
    s = (np.asarray(q, f) @ np.swapaxes(np.asarray(k, f), -1, -2)).astype(f)
    s = np.where(ok, s, f(-np.inf))
    m = s.max(-1, keepdims=True)
    with np.errstate(invalid="ignore"):
        e = (np.exp2(s - m) if exp2 else np.exp(s - m)).astype(f)
    e = np.where(ok, e, f(0))
    return (e * (f(1) / e.sum(-1, keepdims=True, dtype=f))).astype(f)


def emulate(d, exp2, round_p=False, fault=None):
    """The kernels' arithmetic in float32 numpy on the finite arrays of case(): both softmaxes, the gather, (1 - blend) pt + blend ps,
    times gain, optionally rounded to bf16 (the MFMA kernel), P . V accumulated in f32.  fault: None or one of FAULTS --
      map_ignored               no key has a source               map_shifted     every mapped key reads the next source row
      blend_ignored             a mapped key takes the source whole (blend 1)
      blend_swapped             blend and 1 - blend change places
      gain_dropped              gain 1                            source_length_ignored   the source softmax and `has` run over all Ls rows
      target_length_off_by_one  one more target key (one fewer at the full length)
      renormalised              every row of P divided by its sum
      pairs_swapped             pair b runs under pair b ^ 1's controls
      next_head_source          head h blends the source probabilities of head h + 1"""
    assert fault is None or fault in FAULTS, fault
    f = np.float32
    B, H, nq, dh = d["qt"].shape
    Ls, Lt = d["ks"].shape[2], d["kt"].shape[2]
    ns, nt = clamp(d["lens_s"], B, Ls), clamp(d["lens_t"], B, Lt)
    rm, bl, g = d["row_map"].astype(np.int64), d["blend"].astype(f), d["gain"].astype(f)
    if fault == "pairs_swapped":
        idx = np.arange(B) ^ 1
        idx = np.where(idx < B, idx, np.arange(B))
        rm, bl, g = rm[idx], bl[idx], g[idx]
    if fault == "source_length_ignored":
        ns = np.full(B, Ls, np.int64)
    if fault == "target_length_off_by_one":
        nt = np.where(nt < Lt, nt + 1, np.maximum(nt - 1, 1))
    if fault == "map_shifted":
        rm = np.where(rm >= 0, rm + 1, rm)
    if fault == "gain_dropped":
        g = np.ones_like(g)
    ps, pt = _softmax32(d["qs"], d["ks"], ns, exp2), _softmax32(d["qt"], d["kt"], nt, exp2)
    if fault == "next_head_source":
        ps = np.roll(ps, -1, axis=1)
    live = np.arange(Lt)[None, :] < nt[:, None]
    has = live & (rm >= 0) & (rm < ns[:, None]) & (bl != 0)
    if fault == "map_ignored":
        has = np.zeros_like(has)
    if fault == "blend_ignored":
        bl = np.where(has, f(1), bl)
    psm = np.take_along_axis(ps, np.broadcast_to(np.where(has, rm, 0)[:, None, None, :], pt.shape), -1)
    a, c = (bl, (f(1) - bl).astype(f)) if fault == "blend_swapped" else ((f(1) - bl).astype(f), bl)
    mixed = (c[:, None, None, :] * psm + (a[:, None, None, :] * pt).astype(f)).astype(f)
    p = (g[:, None, None, :] * np.where(has[:, None, None, :], mixed, pt)).astype(f)
    p = np.where(live[:, None, None, :], p, f(0))
    if fault == "renormalised":
        with np.errstate(invalid="ignore", divide="ignore"):      # (a row whose every gain is 0 has nothing to divide by)
            p = (p / p.sum(-1, keepdims=True, dtype=f)).astype(f)
    if round_p:
        p = P.bf16_round(p)
    v = np.where(live[:, None, :, None], np.asarray(d["v"], f), f(0))
    return (p @ v).astype(f)


def fault_applies(fault, d):
    """whether the fault changes the arithmetic at all at these inputs (with one source and one target key every probability is 1: the
    map, the blend, the heads and a renormalisation cannot be told apart; without a length array there is no length to get wrong)"""
    B, H = d["qt"].shape[:2]
    Ls, Lt = d["ks"].shape[2], d["kt"].shape[2]
    has, m, w_t, w_s, g = weights(d)
    has = has & (g > 0)                                       # a key with gain 0 shows nothing of its source
    many = Ls >= 2 and Lt >= 2
    wide = clamp(d["lens_s"], B, Ls) >= 2                       # with one source key every head's source probability is 1
    return {"map_ignored": many and bool(has.any()), "map_shifted": many and bool(has.any()), "blend_ignored": many and bool((has & (w_t > 0)).any()),
            "blend_swapped": many and bool((has & (w_t != w_s)).any()), "gain_dropped": bool((g != 1)[w_t + w_s > 0].any()),
            "source_length_ignored": many and d["lens_s"] is not None and bool((clamp(d["lens_s"], B, Ls) < Ls).any()) and bool(has.any()),
            "target_length_off_by_one": Lt >= 2 and d["lens_t"] is not None, "renormalised": Lt >= 2, "pairs_swapped": B >= 2 and Lt >= 2,
            "next_head_source": H >= 2 and many and bool((has.any(1) & wide).any())}[fault]
