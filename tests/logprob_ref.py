"""The token likelihood (pmhip_token_logprob) restated in float64, its inputs, and an element-wise bound.

THE OPERATOR.  Row r is scored iff (ids is None or ids[r] == mask_id) and 0 <= target[r] < V.  With x the row, t its target, m = max x,
s = sum exp(x_i - m):  lp = (x_t - m) - log s;  ent = log s + sum_i p_i (m - x_i) (a -inf column adds nothing);  rk = #{i : x_i > x_t, or
x_i == x_t and i < t}.  A target on a -inf column: lp = -inf.  A NaN in a scored row: lp and ent NaN, rk unspecified.  A scored row stores
(lp, ent, rk, 1) (accumulate: adds them); an unscored row stores (0, 0, 0, 0) (accumulate: untouched).

THE INPUTS (``case(V, variant)``): M = 2 * 4 + 1 = 9 rows -- the narrow classes serve four rows per workgroup, the wide ones one -- of a
seeded family per V.  "Trained-like" is a Gaussian floor (sigma 1) with one dominant class, 8 above it, at the middle column `mid`.
  row 0  trained-like, the target ON the maximum (mid):                  rank 0, the row's largest lp
  row 1  near one-hot: +100 at column V - 2 (the last register group), the target elsewhere: lp ~ -100.  A maximum that leaves the last
         group out overflows the exponential
  row 2  flat (every column 0.375), target V / 2:                         lp = -log V, ent = log V, rank = V / 2 (ties below AND above)
  row 3  nearly flat (sigma 0.05), target 3
  row 4  the floor rounded to halves (duplicates everywhere), the target's value repeated at t - 1, t + 1, t - 2 and t + 5: ties below
         and above its column
  row 5  trained-like, the target ON a -inf column (9), columns 2 and V - 3 -inf too:   lp = -inf, ent finite
  row 6  ONE finite column (the target, V - 1), every other column -inf:  lp = 0 and ent = 0 exactly, rank 0
  row 7  trained-like, one NaN at column V - 5, the target elsewhere:    lp and ent NaN
  row 8  trained-like, the target mid + 1 (V = 4: column 3)
Variant 0 leaves rows 1, 3, 5, 7 unscored, by ids != mask_id; variant 1 rows 0, 2, 4, 6, 8, by: ids, target == mask_id, target == -1,
target == 2^40 + 3 (>= V, and its low 32 bits a valid column), ids.  The logits of every unscored row are NaN in every column: every
kind of row is scored once and skipped once.  Variant 2, THE INDEX PROBES: ids None, rows of small integers, exact in fp32,
    x[r, i] = (i + 2 * (i // 256) + r) mod 5,     target[r] = (r * V) // 9 + r  (mod V)
-- the value changes by a non-zero integer (mod 5: by 1 to 4) from column t to t +- 1 (a lane's neighbour element), t +- 4 (the next
lane), t +- 256 (a row of lanes: 258 = 3 mod 5; the next wave where a row has several), t +- 1024 and t +- 2048 (the next register group
with four and eight waves: 1032 = 2, 2064 = 4 mod 5).  Taking any of these columns for the target moves lp by at least 1, orders of
magnitude above the bound, and with V / 5 ties per value the rank is exact only if every column is compared under its own index.
The padding columns [V, ldl) hold NaN in the GPU test.

THE KERNEL'S LAYOUT (``layout``): a row belongs to W waves, each lane holding G float4 groups; register group g covers the columns
[g * W * 256, (g + 1) * W * 256).

THE BOUND, u = 2^-24 (round to nearest), for a scored row with m exact (a maximum does not round), d_i = x_i - m, w_i = exp(d_i):
  a term     e_i = exp2(rn(rn(x_i - m) * log2e)): the subtraction, the constant and the product round once each (u |d_i| each, in the
             exponent) and the hardware exponential is good to one ulp = 2 u of its result (the figure the HIP programming guide's table
             gives for __expf): e_i is off by at most eps_i = 2 u + 3 u |d_i| of itself (2^-126 absolutely where flushed).
  the sum    no term passes through more than n = G + 2 + 6 + W additions of non-negative numbers (two inside its float4, the lane's
             chain over G groups, six butterfly levels, the waves in order), each off by u of its result:
             rel_s = (sum_i w_i eps_i) / s + gamma_n,   gamma_n = n u / (1 - n u).
  L          = rn(log2(s) ln2): the sum's own error moves log s by rel_s; the hardware logarithm is good to one ulp (2 u of its
             result), the constant and the product round once each:  E_L = rel_s + 4 u log s.
  lp         = rn(rn(x_t - m) - L):  B_lp = (u |d_t| + E_L + u |lp|) (1 + 2^-10) + 2^-100
  T          = sum e_i (-d_i): a term is off by eps_i + 2 u of itself (the rounded d_i, the product), the sum as above:
             E_T = [ sum_i w_i |d_i| (eps_i + 2 u) + gamma_n sum_i w_i |d_i| ] / s
  ent        = rn(L + rn(T / s)): the quotient carries rel_s of the divisor and its own rounding:
             B_ent = (E_L + E_T + (T / s) (rel_s + u) + u ent) (1 + 2^-10) + 2^-100
The factors 1 + 2^-10 cover the products of the small terms, 2^-100 the flushed terms (at most 16384 of 2^-126, times |d_i| < 2^8).
Under `accumulate` the addition to what the output held rounds once more: u |acc0 + v| on top.  ``n_adds`` replaces n for an evaluation
whose sums have another depth (the plain-torch branch of the pipeline: at most V).  Rank and count are integers: exact.
Derived from the kernel's operation count and the formats, never from what a GPU returned.
"""
import numpy as np

F = np.float32
U = 2.0 ** -24
ROWS_PER_WORKGROUP = 4                     # logprob.hip: the narrow classes; the wide ones serve one row per workgroup
M = 2 * ROWS_PER_WORKGROUP + 1
VS = (256, 1024, 8192, 16384, 1000, 4)     # the four classes at their upper ends; 1000 leaves the last register group ragged; 4 = one float4
VARIANTS = (0, 1, 2)
FAULTS = ("neighbouring_column", "entropy_without_the_inf_select", "rank_without_the_column_tie_break", "log2_left_unscaled",
          "last_group_out_of_max", "unscored_row_scored", "count_not_incremented", "accumulate_overwrites")
BIG = 2 ** 40 + 3


def layout(V):
    """(G float4 groups a lane holds, W waves a row belongs to) -- logprob.hip's classes"""
    return (1, 1) if V <= 256 else (4, 1) if V <= 1024 else (8, 4) if V <= 8192 else (8, 8)


def case(V, variant):
    """-> dict(a f32 [M, V], ids int64 [M] or None, mask_id = V, target int64 [M], logp0 / ent0 f32 [M], rank0 / count0 int32 [M]:
    what an accumulating launch finds); read-only arrays"""
    assert variant in VARIANTS
    r9 = np.arange(M)
    if variant == 2:
        i = np.arange(V)
        a = ((i[None] + 2 * (i[None] // 256) + r9[:, None]) % 5).astype(F)
        target = (((r9 * V) // 9 + r9) % V).astype(np.int64)
        ids = None
    else:
        rng = np.random.default_rng([V, 31])
        a = rng.standard_normal((M, V)).astype(F)
        mid = (V // 2) | 1
        target = np.zeros(M, np.int64)
        for r in (0, 5, 7, 8):
            a[r, mid] = 8.0
        target[0] = mid
        a[1, V - 2] = 100.0
        target[1] = V // 3
        a[2] = 0.375
        target[2] = V // 2
        a[3] *= F(0.05)
        target[3] = 3
        a[4] = np.round(a[4] * 2) / 2
        t = min(max(V // 2 - 7, 2), V - 2)
        target[4] = t
        for c in (t - 1, t + 1, t - 2, t + 5):
            if 0 <= c < V:
                a[4, c] = a[4, t]
        a[5, [min(9, V - 1), 2, V - 3]] = -np.inf
        target[5] = min(9, V - 1)
        a[6] = -np.inf
        a[6, V - 1] = 1.25
        target[6] = V - 1
        a[7, max(V - 5, 0)] = np.nan
        target[7] = 1
        target[8] = min(mid + 1, V - 1)
        ids = np.full(M, V, np.int64)
        other = ((r9 * 7 + 3) % V).astype(np.int64)
        if variant == 0:
            unscored = r9 % 2 == 1
            ids[unscored] = other[unscored]
        else:
            unscored = r9 % 2 == 0
            ids[[0, 8]] = other[[0, 8]]
            target[2], target[4], target[6] = V, -1, BIG
        a[unscored] = np.nan
    d = dict(a=a, ids=ids, mask_id=V, target=target, V=V, variant=variant,
             logp0=(-0.25 * (r9 + 1)).astype(F), ent0=(0.5 * (r9 + 1)).astype(F), rank0=(r9 * 5 + 1).astype(np.int32), count0=(r9 + 3).astype(np.int32))
    for x in d.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return d


def scored_rows(ids, mask_id, target, V):
    target = np.asarray(target)
    ok = (target >= 0) & (target < V)
    return ok if ids is None else ok & (np.asarray(ids) == mask_id)


def values(a, target, fault=None):
    """float64 (lp, ent, rk) [rows] of EVERY row whose target is a column (others: 0), by the rules above.  fault: the restatement with
    that mistake built in."""
    a = np.asarray(a, np.float64)
    rows, V = a.shape
    target = np.asarray(target)
    ok = (target >= 0) & (target < V)
    t = np.where(ok, target, 0)
    G, W = layout(V)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = a.max(1)
        if fault == "last_group_out_of_max":
            lastg = np.zeros(V, bool)
            lastg[(G - 1) * W * 256:] = True
            m = np.where(lastg[None], -np.inf, a).max(1)
        d = a - m[:, None]
        w = np.exp(d)
        if fault == "last_group_out_of_max":
            w = w.astype(F).astype(np.float64)                  # the kernel's format: what overflows there does here
        s = w.sum(1)
        L = np.log2(s) if fault == "log2_left_unscaled" else np.log(s)
        tt = np.minimum(t + 1, V - 1) if fault == "neighbouring_column" else t
        xt = a[np.arange(rows), tt]
        lp = (xt - m) - L
        term = w * -d
        if fault != "entropy_without_the_inf_select":
            term = np.where(w == 0, 0.0, term)
        ent = L + term.sum(1) / s
        cols = np.arange(V)[None]
        before = a > xt[:, None]
        if fault != "rank_without_the_column_tie_break":
            before |= (a == xt[:, None]) & (cols < tt[:, None])
        rk = before.sum(1)
    return np.where(ok, lp, 0.0), np.where(ok, ent, 0.0), np.where(ok, rk, 0)


def reference(a, ids, mask_id, target, logp0=None, ent0=None, rank0=None, count0=None, accumulate=False, fault=None):
    """-> (logp, ent float64 [M], rank, count int64 [M], scored bool [M]).  *0: what the outputs held (accumulate only)."""
    V = np.asarray(a).shape[1]
    scored = scored_rows(ids, mask_id, target, V)
    if fault == "unscored_row_scored":
        scored = (np.asarray(target) >= 0) & (np.asarray(target) < V)
    lp, ent, rk = values(a, target, fault=fault)
    if accumulate:
        prev = [np.asarray(x, np.float64 if i < 2 else np.int64) for i, x in enumerate((logp0, ent0, rank0, count0))]
        over = fault == "accumulate_overwrites"
        out = [np.where(scored, v if over else p + v, p) for p, v in zip(prev[:3], (lp, ent, rk))]
        out.append(np.where(scored, prev[3] if fault == "count_not_incremented" else prev[3] + 1, prev[3]))
    else:
        out = [np.where(scored, lp, 0.0), np.where(scored, ent, 0.0), np.where(scored, rk, 0), scored.astype(np.int64)]
    return out[0], out[1], out[2].astype(np.int64), out[3].astype(np.int64), scored


def bound(a, target, logp0=None, ent0=None, n_adds=None):
    """the element-wise bounds (B_lp, B_ent) [M] of the module docstring (0 where the exact result is NaN, inf, or not a scored
    quantity: those are compared exactly).  logp0 / ent0: the bound of an accumulating launch."""
    a = np.asarray(a, np.float64)
    rows, V = a.shape
    G, W = layout(V)
    n = G + 2 + 6 + W if n_adds is None else n_adds
    gamma = n * U / (1 - n * U)
    up = 1 + 2.0 ** -10
    lp, ent, _ = values(a, target)
    target = np.asarray(target)
    t = np.where((target >= 0) & (target < V), target, 0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m = a.max(1)
        d = a - m[:, None]
        w = np.exp(d)
        s = w.sum(1)
        ad = np.where(np.isfinite(d), np.abs(d), 0.0)
        eps = 2 * U + 3 * U * ad
        rel_s = (w * eps).sum(1) / s + gamma
        E_L = rel_s + 4 * U * np.log(s)
        dt = np.abs(d[np.arange(rows), t])
        B_lp = (U * dt + E_L + U * np.abs(lp)) * up + 2.0 ** -100
        wd = w * ad
        E_T = ((wd * (eps + 2 * U)).sum(1) + gamma * wd.sum(1)) / s
        B_ent = (E_L + E_T + wd.sum(1) / s * (rel_s + U) + U * np.abs(ent)) * up + 2.0 ** -100
        B_lp, B_ent = np.where(np.isfinite(lp), B_lp, 0.0), np.where(np.isfinite(ent), B_ent, 0.0)
        for B, v, v0 in ((B_lp, lp, logp0), (B_ent, ent, ent0)):
            if v0 is not None:
                B += U * np.abs(np.asarray(v0, np.float64) + np.where(np.isfinite(v), v, 0.0)) * up
    return B_lp, B_ent


def check(got, want, B, slack=1.0):
    """got = (logp, ent or None, rank or None, count or None) from a kernel or a faulty restatement, want = reference(...), B = bound(...)
    -> (list of failure texts, the worst err / B over the scored finite values).  rank and count exact (the rank of a row whose exact lp
    is NaN is unspecified: not compared); an unscored row's values exact (0, or what they held); NaN for NaN, -inf for -inf and 0 for an
    exact 0, exactly; every other scored value within slack * B."""
    wl, we, wr, wc, scored = want
    fails = []
    if got[3] is not None:
        for r in np.nonzero(np.asarray(got[3]) != wc)[0]:
            fails.append(f"row {r}: count {np.asarray(got[3])[r]} != {wc[r]}")
    if got[2] is not None:
        for r in np.nonzero((np.asarray(got[2]) != wr) & ~np.isnan(wl))[0]:
            fails.append(f"row {r}: rank {np.asarray(got[2])[r]} != {wr[r]}")
    worst = 0.0
    for name, g_all, w_all, Bv in (("logp", got[0], wl, B[0]), ("entropy", got[1], we, B[1])):
        if g_all is None:
            continue
        for r in range(len(w_all)):
            g, w = np.float64(np.asarray(g_all)[r]), w_all[r]
            if np.isnan(w):
                if not np.isnan(g):
                    fails.append(f"row {r}: {name} {g!r} is not NaN")
            elif not scored[r] or np.isinf(w) or w == 0.0:
                if not g == w:
                    fails.append(f"row {r}: {name} {g!r} is not exactly {w!r} ({'scored' if scored[r] else 'unscored'})")
            else:
                err = abs(g - w)
                ratio = np.inf if not np.isfinite(g) else err / Bv[r]
                worst = max(worst, ratio)
                if not ratio < slack:
                    fails.append(f"row {r}: |{name} - {name}64| = {err:.3e} is {ratio:.3g} x the bound {Bv[r]:.3e}")
    return fails, worst


def restate_f32(a, target):
    """the operator's arithmetic in float32 torch, operation for operation (torch's own sums) -> (lp, ent f32 [rows], rk int64 [rows])
    of every row; the targets must be columns"""
    import torch
    a = torch.from_numpy(np.array(a, F))
    t = torch.from_numpy(np.array(target, np.int64))[:, None]
    log2e, ln2 = torch.tensor(1.4426950408889634, dtype=torch.float32), torch.tensor(0.6931471805599453, dtype=torch.float32)
    d = a - a.amax(1, keepdim=True)
    e = torch.exp2(d * log2e)
    e = torch.where(e < 2.0 ** -126, torch.zeros_like(e), e)                # (the hardware exponential returns no subnormals)
    s = e.sum(1)
    L = torch.log2(s) * ln2
    xt = a.gather(1, t)
    lp = d.gather(1, t)[:, 0] - L
    ent = L + torch.where(e == 0, torch.zeros_like(e), e * -d).sum(1) / s
    rk = ((a > xt) | ((a == xt) & (torch.arange(a.shape[1])[None] < t))).sum(1)
    return lp.numpy(), ent.numpy(), rk.numpy()


def neighbours(a, target):
    """What the two kernels that already score a target leave, bounded against float64 for rows WITHOUT -inf or NaN:
      p_forced = 1 - score of pmhip_sample_rows_forced = rn(1 - rn(expf(rn(x_t - m)) / se)),   nll_ce = row_loss of pmhip_masked_ce at
      label_smoothing 0 = rn(rn(m + logf(se)) - x_t)
    Both hold the row in ONE wave of NV4 = 1, 4, 32, 64 float4 groups a lane (V <= 256, 1024, 8192, 16384) and sum se = sum __expf(x_i - m)
    over n' = NV4 + 2 + 6 additions, each term off by eps_i as above (subtraction, the scaled exponent, the exponential):
      rel_s' = (sum w_i eps_i) / s + gamma_n'
      p_forced:  p (eps_t + rel_s' + u) for the quotient, u for each of the two subtractions from 1 (|.| <= 1):
                 B_p = p (eps_t + rel_s' + u) (1 + 2^-10) + 2 u + 2^-126
      nll_ce:    the logarithm (one ulp, 2 u log s, of a sum off by rel_s'), the addition to m, the subtraction of x_t:
                 B_nll = (rel_s' + 2 u log s + u |m + log s| + u |nll|) (1 + 2^-10)
    -> (p float64 [rows], B_p, nll float64 [rows], B_nll)"""
    a = np.asarray(a, np.float64)
    rows, V = a.shape
    assert np.isfinite(a).all()
    t = np.asarray(target)
    nv4 = 1 if V <= 256 else 4 if V <= 1024 else 32 if V <= 8192 else 64
    n = nv4 + 2 + 6
    gamma = n * U / (1 - n * U)
    up = 1 + 2.0 ** -10
    m = a.max(1)
    d = a - m[:, None]
    w = np.exp(d)
    s = w.sum(1)
    eps = 2 * U + 3 * U * np.abs(d)
    rel_s = (w * eps).sum(1) / s + gamma
    dt = d[np.arange(rows), t]
    p = np.exp(dt) / s
    B_p = p * (eps[np.arange(rows), t] + rel_s + U) * up + 2 * U + 2.0 ** -126
    nll = (m + np.log(s)) - a[np.arange(rows), t]
    B_nll = (rel_s + 2 * U * np.log(s) + U * np.abs(m + np.log(s)) + U * np.abs(nll)) * up
    return p, B_p, nll, B_nll
