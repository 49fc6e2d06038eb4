"""The forced step (pmhip_sample_rows_forced) restated in float64, its inputs, and an element-wise bound.

THE STEP.  For row r with logits x, given id c and target t:  pred = t;  merged = t if c == mask_id else c;
score = 1 - exp(x_t - max x) / sum_j exp(x_j - max x) if c == mask_id else -1e5.  A target outside [0, V): pred = merged = c, -1e5.

THE INPUTS (``case(V, variant)``): M = 9 rows -- two workgroups of four waves and one wave of a third -- of a seeded family per V:
  rows 0..5 trained-like: a Gaussian floor (sigma 1) with ONE dominant class; rows 6..8 nearly flat (sigma 0.05).
  row 0  dominant +8 at a middle column,            target column 0
  row 1  dominant +8 at column V - 3 (last group),  target column V - 1
  row 2  dominant +100 at column V - 2,             target the arg-max itself.  The other register groups stay 90 and more below
         it: a maximum that leaves the last group out overflows __expf here (inf / inf), which no shift of the maximum hides.
  row 3  dominant +8,                               target a mid-probability class (+5)
  row 4  dominant +110 at column V - 2,             target a floor class 120 and more below it: expf underflows, p = 0, score = 1
  row 5  dominant +8,                               target a class whose logit is -inf: p = 0, score = 1
  row 6  flat,                                      target column 0
  row 7  flat,                                      target column V - 1
  row 8  flat,                                      target a middle column
Variant 0 gives the odd rows their id (4 of 9), variant 1 the even rows (5 of 9): every kind of row is scored once and skipped once.
A given id differs from the row's target.  The padding columns [V, ldl) hold NaN in the GPU test.

THE BOUND on |score - (1 - p64)| for a scored row, u = 2^-24 (round to nearest), d_j = x_j - max (the maximum itself is exact):
  a term     __expf(d_j) = v_exp_f32(d_j * log2e): the subtraction rounds once (u |d_j| in the exponent), the constant and the product
             once each (u |d_j| each), the hardware exponential is good to one ulp = 2 u of its result -- the figure the HIP
             programming guide's table gives for __expf, and for expf -- so a term is off by at most e_j = 2 u + 3 u |d_j| of itself
             (and by 2^-126 absolutely where the result is flushed).  The numerator expf(x_t - max) gets the same formula.
  the sum    4 * NV4 lane terms and six butterfly levels: no term passes through more than n = 4 * NV4 + 6 additions of non-negative
             numbers, each off by u of its result: the sum is off by at most gamma_n = n u / (1 - n u) of itself, on top of the
             terms' own errors weighted by the terms:  rel_se = (sum_j w_j e_j) / (sum_j w_j) + gamma_n,  w_j = exp(d_j).
  the rest   one division (u of p) and one subtraction (u of 1 - p).
  together   B = p (e_t + rel_se + u) (1 + 2^-10) + u (1 - p) + V 2^-126.  The factor 1 + 2^-10 covers the products of the small terms.
Derived from the kernel's operation count and the formats, never from what a GPU returned.  The block-statistics kernel of the draw
rounds its confidence by another route (sample.hip); against it the issue's figure applies: twice this bound.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
ROWS_PER_WORKGROUP = 4                     # sample.hip: THREADS / 64
M = 2 * ROWS_PER_WORKGROUP + 1
VS = (64, 1000, 8192, 16384)               # the four NV4 classes; 1000 is no multiple of 64 or 256
GIVEN_SCORE = F(-1e5)
FAULTS = ("target_off_by_one", "top5_normaliser", "last_group_out_of_max", "last_group_out_of_sum", "p_for_one_minus_p", "given_row_scored",
          "given_id_overwritten")


def nv4(V):
    return 1 if V <= 256 else 4 if V <= 1024 else 32 if V <= 8192 else 64


def case(V, variant):
    """-> dict(logits f32 [M, V], ids int64 [M], target int64 [M], mask_id = V); read-only arrays"""
    rng = np.random.default_rng([V, 17])
    x = rng.standard_normal((M, V)).astype(F)
    x[6:] *= F(0.05)
    mid = (V // 2) | 1
    target = np.zeros(M, np.int64)
    x[0, mid] = 8.0
    target[0] = 0
    x[1, V - 3] = 8.0
    target[1] = V - 1
    x[2, V - 2] = 100.0
    target[2] = V - 2
    x[3, mid] = 8.0
    x[3, mid + 2] = 5.0
    target[3] = mid + 2
    x[4, V - 2] = 110.0
    x[4, 5] = -10.5
    target[4] = 5
    x[5, mid] = 8.0
    x[5, 9] = -np.inf
    target[5] = 9
    target[6], target[7], target[8] = 0, V - 1, mid
    given = (np.arange(M) % 2 == 1) if variant == 0 else (np.arange(M) % 2 == 0)
    ids = np.where(given, (target + 3) % V, V).astype(np.int64)
    d = dict(logits=x, ids=ids, target=target, mask_id=V, V=V, variant=variant)
    for a in (x, ids, target):
        a.setflags(write=False)
    return d


def reference(logits, ids, target, mask_id, fault=None):
    """the float64 restatement -> (pred int64 [M], merged int64 [M], score float64 [M] (-1e5 at given ids), p float64 [M]).
    fault: one of FAULTS -- the restatement with that mistake built in (tests/test_forced_cpu.py proves the bound sees each)"""
    x = np.asarray(logits, np.float64)
    rows, V = x.shape
    ids, target = np.asarray(ids, np.int64), np.asarray(target, np.int64)
    ok = (target >= 0) & (target < V)
    t = np.where(ok, target, 0)
    if fault == "target_off_by_one":
        t = (t + 1) % V
    lastg = np.zeros(V, bool)
    lastg[(nv4(V) - 1) * 256:] = True                      # the columns of register group NV4 - 1: (g * 64 + lane) * 4 + e
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        mx = np.where(lastg[None, :], -np.inf, x).max(1) if fault == "last_group_out_of_max" else x.max(1)
        w = np.exp(x - mx[:, None])
        if fault == "last_group_out_of_max":
            w = w.astype(F).astype(np.float64)             # the kernel's format: what overflows there overflows here
        if fault == "top5_normaliser":
            se = np.sort(w, axis=1)[:, -5:].sum(1)
        elif fault == "last_group_out_of_sum":
            se = np.where(lastg[None, :], 0.0, w).sum(1)
        else:
            se = w.sum(1)
        p = w[np.arange(rows), t] / se
    given = ids != mask_id
    take = ok & ~given
    score = np.where(take, p if fault == "p_for_one_minus_p" else 1.0 - p, np.float64(GIVEN_SCORE))
    if fault == "given_row_scored":
        score = np.where(ok, 1.0 - p, score)
    pred = np.where(ok, target, ids)
    merged = np.where(take, target, ids)
    if fault == "given_id_overwritten":
        merged = np.where(ok, target, ids)
    return pred, merged, score, np.where(ok, p, 0.0)


def bound(logits, target):
    """the element-wise bound B [M] of the module docstring, for the scored rows (a row whose target is out of range gets 0: its
    -1e5 is exact)"""
    x = np.asarray(logits, np.float64)
    rows, V = x.shape
    target = np.asarray(target, np.int64)
    ok = (target >= 0) & (target < V)
    t = np.where(ok, target, 0)
    n_add = 4 * nv4(V) + 6
    gamma = n_add * U / (1 - n_add * U)
    with np.errstate(invalid="ignore"):
        d = x - x.max(1, keepdims=True)
        w = np.exp(d)
        e = 2 * U + 3 * U * np.where(np.isfinite(d), np.abs(d), 0.0)       # (a -inf logit: its term is exactly 0)
    rel_se = (w * e).sum(1) / w.sum(1) + gamma
    r = np.arange(rows)
    p = w[r, t] / w.sum(1)
    B = p * (e[r, t] + rel_se + U) * (1 + 2.0 ** -10) + U * (1 - p) + V * 2.0 ** -126
    return np.where(ok, B, 0.0)


def check(got, want, B, slack=1.0):
    """got = (pred, merged, score) from a kernel or a faulty restatement, want = reference(...)[:3] -> (list of failure texts, the
    worst err / B over the scored rows).  pred / merged exact; a -1e5 exact; a score within slack * B of 1 - p64; NaN fails."""
    pred, merged, score = (np.asarray(a) for a in got)
    wp, wm, ws = want
    fails = []
    for r in np.nonzero(pred != wp)[0]:
        fails.append(f"row {r}: pred {pred[r]} != {wp[r]}")
    for r in np.nonzero(merged != wm)[0]:
        fails.append(f"row {r}: merged {merged[r]} != {wm[r]}")
    worst = 0.0
    for r in range(len(ws)):
        s = np.float64(score[r])
        if ws[r] == np.float64(GIVEN_SCORE):
            if not (F(score[r]) == GIVEN_SCORE):
                fails.append(f"row {r}: score {s!r} is not the exact -1e5 of a given id")
            continue
        err = abs(s - ws[r])
        ratio = np.inf if not np.isfinite(s) else err / B[r]
        worst = max(worst, ratio)
        if not ratio < slack:
            fails.append(f"row {r}: |score - (1 - p64)| = {err:.3e} is {ratio:.3g} x the bound {B[r]:.3e}")
    return fails, worst
