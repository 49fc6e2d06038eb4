"""The logit divergence (pmhip_logit_divergence) restated in float64, its inputs, and an element-wise bound.

THE OPERATOR.  Row r is scored iff ids is None or ids[r] == mask_id.  With p = softmax(a_r), q = softmax(b_r), each over its own row:
tv d = 1/2 sum |p_i - q_i|; jeffreys d = sum (p_i - q_i)(log p_i - log q_i).  A column -inf in both rows adds nothing, -inf in one row
makes jeffreys +inf, a NaN in a scored row makes its result NaN.  A scored row: acc = d, count = 1 (accumulate: acc += d, count += 1);
an unscored row: acc = 0, count = 0 (accumulate: both untouched).

THE INPUTS (``case(V, kind, variant)``): M = 2 * 4 + 1 = 9 row pairs -- the narrow classes serve four pairs per workgroup, the wide ones
one -- of a seeded family per V (the same rows for both kinds).  "Trained-like" is a Gaussian floor (sigma 1) with one dominant class.
  row 0  trained-like, b == a bit for bit:                           exactly 0
  row 1  trained-like, b = a + 37.5 in every column:                 softmax does not see the shift; the value lies within the bound of what the
         rounded sums leave (a maximum shared by the two rows, or none, has to carry 37.5 and more in every exponent)
  row 2  a: dominant +100 at column V - 2 (the last register group), b: a floor around -15 with its dominant class 8 above it at a
         middle column.  tv ~ 1.  A maximum that leaves the last group out overflows the exponential (inf / inf); a maximum shared
         by the rows sends every term of b below the smallest float32 (0 / 0)
  row 3  two nearly flat rows (sigma 0.05), b = a + 0.01 N(0, 1):   the cancellation regime, p - q three orders below p
  row 4  trained-like pair, the same arg-max (+8 and +7.5), different tails
  row 5  as row 4, column 9 -inf in BOTH rows:                       the column adds nothing
  row 6  as row 4, column 9 -inf in a only:                          jeffreys exactly +inf, tv finite
  row 7  as row 4, one NaN in b (column V - 5):                      NaN
  row 8  NaN in every column of both rows:                           NaN when scored; skipped, it must reach nothing
Variant 0 scores the odd rows (ids == mask_id there), variant 1 the even ones: every kind of row is scored once and skipped once.  The
padding columns [V, ldl) hold NaN in the GPU test.

THE KERNEL'S LAYOUT (``layout``): a row pair belongs to W waves, each lane holding G float4 groups of both rows; register group g
covers the columns [g * W * 256, (g + 1) * W * 256).

THE BOUND on |d - d64| for a scored row, u = 2^-24 (round to nearest).  Per row x with maximum m (exact), d_i = x_i - m, w_i = exp(d_i):
  a term     e_i = exp2(rn(rn(x_i - m) * log2e)): the subtraction, the constant and the product round once each (u |d_i| each, in the
             exponent) and the hardware exponential is good to one ulp = 2 u of its result -- the figure the HIP programming guide's
             table gives for __expf -- so e_i is off by at most eps_i = 2 u + 3 u |d_i| of itself (2^-126 absolutely where flushed).
  the sum    no term passes through more than n = G + 2 + 6 + W additions of non-negative numbers (two inside its float4, the lane's
             chain over G groups, six butterfly levels, the waves in order), each off by u of its result: the sum is off by at most
             gamma_n = n u / (1 - n u) of itself on top of the terms' own errors:  rel_s = (sum_i w_i eps_i) / (sum_i w_i) + gamma_n.
  p_i        one division for 1 / s and one product: p_i is off by rho_i = eps_i + rel_s + 2 u of itself.
  p_i - q_i  EP_i = (p_i rho^a_i + q_i rho^b_i) (1 + 2^-10) + u |p_i - q_i| + 2^-125       (the subtraction rounds once)
  tv         B = 1/2 [ sum_i EP_i + gamma_n sum_i |p_i - q_i| ] (1 + 2^-10)                  (|.| and the 1/2 are exact)
  jeffreys   its second factor L_i = (d^a_i - d^b_i) - (log s_a - log s_b) carries the cancellation: two subtractions of rounded
             differences, u (|d^a_i| + |d^b_i| + |d^a_i - d^b_i|); the two logarithms, each of a sum that is off by rel_s and then good
             to one ulp, rel_s^a + rel_s^b + 2 u (|log s_a| + |log s_b|); their difference and the last subtraction, u |log s_a - log s_b|
             + u |L_i|.  Call the total EL_i.  The product rounds once and the sum as above:
             B = [ sum_i (EP_i |L_i| + |p_i - q_i| EL_i + EP_i EL_i) + (u + gamma_n) sum_i |p_i - q_i| |L_i| ] (1 + 2^-10)
             -- the error scales with sum |p - q| |log p - log q| and with sum p |log p - log q|, not with d.
The factors 1 + 2^-10 cover the products of the small terms.  Under `accumulate` the addition to what acc held rounds once more:
u |acc0 + d| on top.  Derived from the kernel's operation count and the formats, never from what a GPU returned.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
PAIRS_PER_WORKGROUP = 4                    # divergence.hip: the narrow classes; the wide ones serve one pair per workgroup
M = 2 * PAIRS_PER_WORKGROUP + 1
VS = (64, 1000, 8192, 16384)               # the four classes; 1000 is no multiple of 64 or 256
KINDS = ("tv", "jeffreys")
FAULTS = ("shared_max", "last_group_out_of_max", "last_group_out_of_sum", "kl_for_jeffreys", "tv_without_half", "b_row_off_by_one",
          "unscored_row_scored", "count_not_incremented", "accumulate_overwrites")
SHIFT = 37.5


def layout(V, kind):
    """(G float4 groups a lane holds of each row, W waves a pair belongs to) -- divergence.hip's classes"""
    G, W = (1, 1) if V <= 256 else (4, 1) if V <= 1024 else (8, 4) if V <= 8192 else (8, 8)
    return (4, 2 * W) if kind == "jeffreys" and G == 8 else (G, W)


def case(V, kind, variant):
    """-> dict(a, b f32 [M, V], ids int64 [M], mask_id = V, acc0 f32 [M], count0 int32 [M]: what an accumulating launch finds);
    read-only arrays.  The rows do not depend on the kind."""
    assert kind in KINDS and variant in (0, 1)
    rng = np.random.default_rng([V, 29])
    a = rng.standard_normal((M, V)).astype(F)
    tail = rng.standard_normal((M, V)).astype(F)
    mid = (V // 2) | 1
    b = a.copy()
    a[0, mid] = 8.0
    b[0] = a[0]
    a[1, mid] = 8.0
    b[1] = a[1] + F(SHIFT)
    b[2] = tail[2] - F(15.0)
    a[2, V - 2] = 100.0
    b[2, mid] = -7.0
    a[3] *= F(0.05)
    b[3] = a[3] + F(0.01) * tail[3]
    for r in (4, 5, 6, 7):
        b[r] = F(0.8) * a[r] + F(0.6) * tail[r]
        a[r, mid], b[r, mid] = 8.0, 7.5
    a[5, 9] = b[5, 9] = -np.inf
    a[6, 9] = -np.inf
    b[7, V - 5] = np.nan
    a[8] = b[8] = np.nan
    scored = (np.arange(M) % 2 == 1) if variant == 0 else (np.arange(M) % 2 == 0)
    ids = np.where(scored, V, (np.arange(M) * 7 + 3) % V).astype(np.int64)
    acc0 = (0.25 * np.arange(1, M + 1)).astype(F)
    count0 = (np.arange(M) + 3).astype(np.int32)
    d = dict(a=a, b=b, ids=ids, mask_id=V, acc0=acc0, count0=count0, V=V, kind=kind, variant=variant)
    for x in (a, b, ids, acc0, count0):
        x.setflags(write=False)
    return d


def _softmax_parts(x, m):
    """x float64 [rows, V], m [rows] -> (d, w, s): shifted logits, exp of them (0 at -inf), their sum"""
    with np.errstate(over="ignore", invalid="ignore"):
        d = x - m[:, None]
        w = np.exp(d)
    return d, w, w.sum(1)


def _in_f32(w):
    """float64 terms as the float32 exponential instruction leaves them: rounded, inf above the range, 0 below 2^-126 (it returns no
    subnormals)"""
    w = w.astype(F).astype(np.float64)
    return np.where(w < 2.0 ** -126, 0.0, w)


def divergence(a, b, kind, fault=None):
    """float64 d [rows] of every row pair (NaN / inf by the rules above).  fault: the restatement with that mistake built in."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    rows, V = a.shape
    if fault == "b_row_off_by_one":
        b = np.roll(b, -1, axis=0)
    G, W = layout(V, kind)
    lastg = np.zeros(V, bool)
    lastg[(G - 1) * W * 256:] = True
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ma, mb = a.max(1), b.max(1)
        if fault == "last_group_out_of_max":
            ma, mb = np.where(lastg[None], -np.inf, a).max(1), np.where(lastg[None], -np.inf, b).max(1)
        if fault == "shared_max":
            ma = mb = np.maximum(ma, mb)
        da, wa, _ = _softmax_parts(a, ma)
        db, wb, _ = _softmax_parts(b, mb)
        if fault in ("last_group_out_of_max", "shared_max"):
            wa, wb = _in_f32(wa), _in_f32(wb)                 # the kernel's format: what over- or underflows there does here
        if fault == "last_group_out_of_sum":
            sa, sb = np.where(lastg[None], 0.0, wa).sum(1), np.where(lastg[None], 0.0, wb).sum(1)
        else:
            sa, sb = wa.sum(1), wb.sum(1)
        p, q = wa / sa[:, None], wb / sb[:, None]
        if kind == "tv":
            d = np.abs(p - q).sum(1) * (1.0 if fault == "tv_without_half" else 0.5)
        else:
            L = (da - db) - (np.log(sa) - np.log(sb))[:, None]
            t = (p if fault == "kl_for_jeffreys" else p - q) * L
            gone_a, gone_b = np.isneginf(a), np.isneginf(b)
            t = np.where(gone_a & gone_b, 0.0, t)
            t = np.where(gone_a != gone_b, np.inf, t)
            d = t.sum(1)
    return d


def reference(a, b, ids, mask_id, kind, acc0=None, count0=None, accumulate=False, fault=None):
    """-> (acc float64 [M], count int64 [M], scored bool [M]).  acc0 / count0: what the outputs held (accumulate only)."""
    rows = np.asarray(a).shape[0]
    scored = np.ones(rows, bool) if ids is None else np.asarray(ids) == mask_id
    d = divergence(a, b, kind, fault=fault)
    if fault == "unscored_row_scored":
        scored = np.ones(rows, bool)
    if accumulate:
        acc0, count0 = np.asarray(acc0, np.float64), np.asarray(count0, np.int64)
        acc = np.where(scored, d if fault == "accumulate_overwrites" else acc0 + d, acc0)
        count = np.where(scored, count0 if fault == "count_not_incremented" else count0 + 1, count0)
    else:
        acc = np.where(scored, d, 0.0)
        count = scored.astype(np.int64)
    return acc, count, scored


def bound(a, b, kind, acc0=None):
    """the element-wise bound B [M] of the module docstring (0 where the exact result is NaN, inf or exactly 0 by identity: those
    are compared exactly).  acc0: the bound of an accumulating launch."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    rows, V = a.shape
    G, W = layout(V, kind)
    n = G + 2 + 6 + W
    gamma = n * U / (1 - n * U)
    up = 1 + 2.0 ** -10
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        parts = []
        for x in (a, b):
            d, w, s = _softmax_parts(x, x.max(1))
            eps = 2 * U + 3 * U * np.where(np.isfinite(d), np.abs(d), 0.0)
            rel_s = (w * eps).sum(1) / s + gamma
            parts.append((d, w / s[:, None], s, rel_s, eps + rel_s[:, None] + 2 * U))
        (da, p, sa, rsa, rhoa), (db, q, sb, rsb, rhob) = parts
        EP = (p * rhoa + q * rhob) * up + U * np.abs(p - q) + 2.0 ** -125
        if kind == "tv":
            B = 0.5 * (EP.sum(1) + gamma * np.abs(p - q).sum(1)) * up
        else:
            both = np.isfinite(da) & np.isfinite(db)
            lsa, lsb = np.log(sa), np.log(sb)
            L = np.where(both, (da - db) - (lsa - lsb)[:, None], 0.0)
            EL = (U * (np.abs(da) + np.abs(db) + np.abs(da - db)) + (rsa + rsb + 2 * U * (np.abs(lsa) + np.abs(lsb)) + U * np.abs(lsa - lsb))[:, None]
                  + U * np.abs(L))
            EL = np.where(both, EL, 0.0)
            dp = np.where(both, np.abs(p - q), 0.0)
            B = ((np.where(both, EP, 0.0) * np.abs(L) + dp * EL + np.where(both, EP, 0.0) * EL).sum(1) + (U + gamma) * (dp * np.abs(L)).sum(1)) * up
        d = divergence(a, b, kind)
        B = np.where(np.isfinite(d), B, 0.0)
        if acc0 is not None:
            B = B + U * np.abs(np.asarray(acc0, np.float64) + np.where(np.isfinite(d), d, 0.0)) * up
    return B


def check(got, want, B, slack=1.0):
    """got = (acc, count or None) from a kernel or a faulty restatement, want = reference(...) -> (list of failure texts, the worst
    err / B over the scored finite rows).  count exact; an unscored row's acc exact (0, or what it held); NaN for NaN, +inf for +inf
    and 0 for an exact 0, exactly; every other scored row within slack * B."""
    acc, count = np.asarray(got[0]), got[1]
    wa, wc, scored = want
    fails = []
    if count is not None:
        for r in np.nonzero(np.asarray(count) != wc)[0]:
            fails.append(f"row {r}: count {np.asarray(count)[r]} != {wc[r]}")
    worst = 0.0
    for r in range(len(wa)):
        g = np.float64(acc[r])
        if not scored[r] or np.isinf(wa[r]) or wa[r] == 0.0:
            if not g == wa[r]:
                fails.append(f"row {r}: acc {g!r} is not exactly {wa[r]!r} ({'scored' if scored[r] else 'unscored'})")
        elif np.isnan(wa[r]):
            if not np.isnan(g):
                fails.append(f"row {r}: acc {g!r} is not NaN")
        else:
            err = abs(g - wa[r])
            ratio = np.inf if not np.isfinite(g) else err / B[r]
            worst = max(worst, ratio)
            if not ratio < slack:
                fails.append(f"row {r}: |acc - d64| = {err:.3e} is {ratio:.3g} x the bound {B[r]:.3e}")
    return fails, worst


def restate_f32(a, b, kind):
    """the operator's arithmetic in float32 torch, operation for operation (torch's own sums): -> f32 [rows]"""
    import torch
    a, b = torch.from_numpy(np.array(a, F)), torch.from_numpy(np.array(b, F))
    log2e = torch.tensor(1.4426950408889634, dtype=torch.float32)
    da, db = a - a.amax(1, keepdim=True), b - b.amax(1, keepdim=True)
    ea, eb = torch.exp2(da * log2e), torch.exp2(db * log2e)
    sa, sb = ea.sum(1, keepdim=True), eb.sum(1, keepdim=True)
    dp = ea * (1 / sa) - eb * (1 / sb)
    if kind == "tv":
        return (0.5 * dp.abs().sum(1)).numpy()
    t = dp * ((da - db) - (sa.log() - sb.log()))
    gone_a, gone_b = torch.isneginf(a), torch.isneginf(b)
    t = torch.where(gone_a & gone_b, torch.zeros_like(t), t)
    return torch.where(gone_a != gone_b, torch.full_like(t, float("inf")), t).sum(1).numpy()
