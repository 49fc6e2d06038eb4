"""Probes for the row kernels (paintmind_amd/csrc/rowops.hip) and the loss kernels (paintmind_amd/csrc/loss.hip): inputs on which a
kernel with subtly wrong arithmetic or indexing gives another answer, float64 references built from exactly what the kernel is given,
element-wise bounds derived from the kernel's arithmetic, and float32 numpy restatements (`emulate_*`) that follow the kernel's
summation order and in which faults can be planted one at a time (tests/test_rowop_probes_cpu.py proves that each is rejected;
tests/test_gpu_rowop_probes.py holds the kernels to the same comparisons).  numpy only; not a conftest, not collected.

u = 2^-24 (float32 round to nearest), g(n) = n u / (1 - n u) bounds the compound error of n roundings.

LayerNorm group (layernorm_kernel, hilo_rows_kernel): nv = ceil(D / 256) float4 groups per lane, y = (x - mean) rstd gamma + beta.
    mean   two additions inside the float4, nv lane-serial additions, 6 wave levels, 1 / D rounded, the product     c2 = nv + 10
           |d mean| <= g(c2) max|x_r|;  it moves y by t |gamma_j| with t = g(c2) max|x_r| rstd, and, through the variance
           (sum (x - mean')^2 = sum (x - mean)^2 + D dmean^2), rstd by at most t^2 / 2: the term t^2 |y - beta|
    rstd   x - mean (counts twice in the square), the square, 2 + nv + 6 additions, 1 / D and the product, + eps: nv + 14 roundings
           of var + eps, halved by the square root; the square root and the division                                 nv / 2 + 9
    y      x - mean, rstd, the two products                                                                           c1 = nv / 2 + 12
           the final addition                                                                                         u |y|
    bound = g(c1) |y - beta| + t |gamma_j| + t^2 |y - beta| + u |y|               (contracted multiply-adds round less often)
  An input that is itself computed (x = hi + lo + shift: two additions) adds e_in = u (max|hi + lo| + max|x|) per element: y moves by
  e_in rstd |gamma_j| directly, as much through the mean, and rstd by a factor e_in rstd at most: e_in rstd (2 |gamma_j| + |y - beta|).
  bf16 output: + half an ulp of bf16 at |y| + bound.  bf16 keeps 8 significant bits, so half an ulp of v is 2^-9 times v ROUNDED UP
  TO A POWER OF TWO -- between 2^-9 v and 2^-8 v; `2^-9 |y|` alone is not a bound: 1 + 2^-8 + 2^-20 rounds to 1 + 2^-7, an error of
  (1 - 2^-12) 2^-8 (test_rowop_probes_cpu.py::test_bf16_half_ulp).  hi/lo pair: + 2^-17 (|y| + bound) -- hi takes 8 bits, the
  remainder is exact in float32, smaller than half an ulp of hi unless it is that power of two itself, and lo keeps 8 bits of it.

ln_coef (ln_coef_kernel, the hi plane alone, 8 columns per lane and chunk, two chunks): mean: 3 + 2 + 6 + 2 = 13 roundings; rstd:
(2 + 1 + 16 + 6 + 2 + 1) / 2 + 2 = 16.  coef0 = rstd: rstd (g(16) + t^2);  coef1 = -rstd mean: t + |coef1| (g(17) + t^2), t as above.

ln_coef_parts (common.h lnp_*: every operation explicitly rounded, a fixed tree): the restatement has the kernel's bits up to the
square root, which is the hardware's one-ulp v_sqrt_f32 on the GPU (__fsqrt_rn, unless the toolchain is told to round it), and the
GPU test compares bits around it (parts_bits_match).  The float64 bound holds the reference too: dm = g(5) sum|s_p| / D for the mean;
dM2 = 128 dm sum|d_p| + 64 nparts dm^2 + g(7) M2; rstd relative dM2 rstd^2 / (2 D) + 4 u (M2 / D and + eps halved, the square root's
ulp = 2 u, the division).

masked_ce (one wave per row, NV4 float4 groups per lane): w = sum_j softmax_j |x_j - max| (the product x log2(e) in front of the
hardware exponential loses |x - max| u), lse = max + log(se):
    d lse    = g(w + 3 + NV4 + 8) + 2 u |log se| + u |lse|
    d nll    = d lse + u |nll|                       d smooth = d lse + g(NV4 + 10) mean|x| + u |smooth|
    d row    = ((1 - eps)(d nll + 2 u |nll|) + eps (d smooth + u |smooth|) + u |row|) mask
    d loss   = sum(d row) / sum(mask) + u |loss|     (the reduction is in double)
so the bound scales with max|x| u: 1.8e-4 per row at logits near -3000.

Worst measured ratio |error| / bound per entry over every case the GPU file launches: of the clean restatement
(test_rowop_probes_cpu.py asserts each is at most 1 and prints them), and of the kernels on an MI355X.  The ratios near 1 are the
last rounding alone (u |y|, u |hi + lo|, half an ulp of bf16, 2^-17 |x|), which is attained.
                        restatement   MI355X                              restatement   MI355X
    layernorm f32          0.822      0.822        layernorm bf16            1.000      1.000
    layernorm_hilo f32     0.816      0.816        layernorm_hilo bf16       1.000      1.000
    layernorm_to_hilo      0.970      0.970        split_hilo                0.998      0.998
    join_hilo              1.000      1.000        unshift_hilo              0.950      0.950
    ln_coef                0.215      0.138        ln_coef_parts             0.385      0.410
    masked_ce rows         0.667      0.667        masked_ce loss            0.634      0.634
"""
import numpy as np

from vq_probes import fmaf

F = np.float32
F64 = np.float64
U = 2.0 ** -24
EPS_VALUES = (1e-6, 1e-5, 1e-2)

LN_FAULTS = ("one_pass_variance", "eps_outside_sqrt", "eps_ignored", "unbiased_variance", "stats_from_next_row", "tail_columns_dropped",
             "divide_by_padded_width", "gamma_shifted_4")
HILO_FAULTS = ("lo_plane_ignored", "shift_ignored", "shift_from_next_row")
PARTS_FAULTS = ("upper_parts_dropped", "width_taken_as_1024", "part_means_not_recentred")
CE_FAULTS = ("no_max_subtraction", "smoothing_mean_over_padded_width", "eps_weights_swapped", "mean_over_all_rows", "label_from_next_row")
MASK_FAULTS = ("ties_to_larger_index", "rank_off_by_one", "token_column_from_row")


def g(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16 in numpy (round to nearest even, what torch's cast and the hardware's v_cvt_pk_bf16_f32 do); finite values only
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16_round(x):
    b = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return r.astype(np.uint32).view(F)


def split_hilo(x):
    """the kernel's split: hi = bf16(x), lo = bf16(x - hi) (the difference is exact in float32)"""
    x = np.asarray(x, dtype=F)
    hi = bf16_round(x)
    return hi, bf16_round(x - hi)


def half_ulp_bf16(v):
    """half an ulp of bf16 at magnitude v: 2^-9 times v rounded up to a power of two (0 at 0)"""
    v = np.abs(np.asarray(v, dtype=F64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(v > 0, v, 1.0)))
    return np.where(v > 0, 2.0 ** (e - 8), 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# row families of the LayerNorm group
# ---------------------------------------------------------------------------------------------------------------------------------
# 13 rows: neighbours differ in mean or spread by orders of magnitude, so a statistic taken from the next row shows
ROW_KINDS = ("plain_1", "offset_p1000", "tiny", "constant", "spike_0", "plain_1e-3", "offset_m1000", "plain_1e3", "offset_m30",
             "spike_255", "spike_256", "spike_last", "plain_1")


def make_row(kind, D, rng):
    n = rng.standard_normal(D)
    if kind.startswith("plain_"):
        return float(kind[6:]) * n
    if kind == "offset_p1000":
        return 1000.0 + n
    if kind == "offset_m1000":
        return -1000.0 + n
    if kind == "offset_m30":
        return -30.0 + 0.01 * n
    if kind == "tiny":
        return 1e-3 * n
    if kind == "constant":
        return np.full(D, 0.1)
    if kind.startswith("spike_"):
        col = {"0": 0, "255": min(255, D - 1), "256": 256 % D, "last": D - 1}[kind[6:]]
        n[col] = 1e4
        return n
    raise ValueError(kind)


def row_kinds(M):
    """M = 1: the row that is hardest on the statistics (mean -30, sigma 0.01); else the 13 kinds in turn"""
    return ("offset_m30",) if M == 1 else tuple(ROW_KINDS[i % len(ROW_KINDS)] for i in range(M))


def ln_family(M, D, seed=0):
    """-> dict(x f32 [M, D], gamma, beta f32 [D], kinds).  gamma and beta random, every column its own value, gamma of either sign"""
    rng = np.random.default_rng(1000 * D + 10 * M + seed)
    kinds = row_kinds(M)
    x = np.stack([make_row(k, D, rng) for k in kinds]).astype(F)
    gamma = (rng.uniform(0.5, 1.5, D) * rng.choice([-1.0, 1.0], D)).astype(F)
    beta = rng.standard_normal(D).astype(F)
    return dict(x=x, gamma=gamma, beta=beta, kinds=kinds)


def hilo_family(M, D, seed=0, centred=False):
    """the planes of ln_family's rows.  centred: the pair holds x - shift[row], shift = the row's mean rounded to float32 (the
    centred stream of gemm_common.h); shift differs from row to row by up to 2000.  -> the family plus hi, lo, shift (or None)"""
    fam = ln_family(M, D, seed)
    x = fam["x"]
    if centred:
        shift = x.astype(F64).mean(1).astype(F)
        shift[::5] = 0.0                                       # some rows not centred at all
        hi, lo = split_hilo((x.astype(F64) - shift[:, None].astype(F64)).astype(F))
    else:
        shift = None
        hi, lo = split_hilo(x)
    return dict(fam, hi=hi, lo=lo, shift=shift)


def mixed_magnitudes(M, D, seed=0):
    """rows that mix magnitudes 1e-6 and 1e4 (and both signs) column by column: split / join"""
    rng = np.random.default_rng(77 + 1000 * D + M + seed)
    mag = np.where(rng.random((M, D)) < 0.5, 1e-6, 1e4)
    return (mag * rng.uniform(0.5, 2.0, (M, D)) * rng.choice([-1.0, 1.0], (M, D))).astype(F)


def hilo_value(hi, lo, shift=None):
    """float64 hi + lo (+ shift[row]): what a hi/lo entry is given"""
    x = np.asarray(hi, dtype=F64) + np.asarray(lo, dtype=F64)
    return x if shift is None else x + np.asarray(shift, dtype=F64)[:, None]


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 references and bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_stats(x64, eps):
    x64 = np.asarray(x64, dtype=F64)
    mean = x64.mean(1, keepdims=True)
    var = ((x64 - mean) ** 2).mean(1, keepdims=True)
    return mean, 1.0 / np.sqrt(var + F64(F(eps)))              # the kernel is handed float(eps)


def ln_ref(x64, gamma, beta, eps):
    """two-pass float64 LayerNorm (biased variance, eps inside the square root)"""
    x64 = np.asarray(x64, dtype=F64)
    mean, rstd = ln_stats(x64, eps)
    return (x64 - mean) * rstd * np.asarray(gamma, dtype=F64) + np.asarray(beta, dtype=F64)


def ln_bound(x64, gamma, beta, eps, out="f32", e_in=None):
    """element-wise bound of the module docstring; out: 'f32', 'bf16' or 'hilo'; e_in [M]: error of a computed input"""
    x64 = np.asarray(x64, dtype=F64)
    D = x64.shape[1]
    nv = -(-D // 256)
    c1, c2 = nv / 2 + 12, nv + 10
    ga, be = np.abs(np.asarray(gamma, dtype=F64)), np.asarray(beta, dtype=F64)
    _, rstd = ln_stats(x64, eps)
    y = ln_ref(x64, gamma, beta, eps)
    ymb = np.abs(y - be)
    t = g(c2) * np.abs(x64).max(1, keepdims=True) * rstd
    b = g(c1) * ymb + t * ga + t * t * ymb
    if e_in is not None:
        b = b + np.asarray(e_in, dtype=F64).reshape(-1, 1) * rstd * (2 * ga + ymb)
    b = b + U * (np.abs(y) + b)
    if out == "bf16":
        b = b + half_ulp_bf16(np.abs(y) + b)
    elif out == "hilo":
        b = b + 2.0 ** -17 * (np.abs(y) + b)
    elif out != "f32":
        raise ValueError(out)
    return b


def hilo_input_error(hi, lo, shift=None):
    """e_in [M] of x = fl(fl(hi + lo) + shift): u max|hi + lo| + u max|x| (0 + the first term alone without a shift)"""
    s = np.abs(hilo_value(hi, lo)).max(1)
    return U * s if shift is None else U * s + U * np.abs(hilo_value(hi, lo, shift)).max(1)


def split_bound(x64):
    return 2.0 ** -17 * np.abs(np.asarray(x64, dtype=F64))


def join_bound(hi, lo):
    return U * np.abs(hilo_value(hi, lo))


def unshift_bound(hi, lo, shift):
    """split(fl(fl(hi + lo) + shift)) against float64 hi + lo + shift"""
    e = hilo_input_error(hi, lo, shift)[:, None]
    return e + 2.0 ** -17 * (np.abs(hilo_value(hi, lo, shift)) + e)


def coef_ref(x64, eps):
    """(rstd, -rstd mean) [M, 2] in float64"""
    mean, rstd = ln_stats(x64, eps)
    return np.concatenate([rstd, -rstd * mean], axis=1)


def coef_bound(x64, eps):
    x64 = np.asarray(x64, dtype=F64)
    mean, rstd = ln_stats(x64, eps)
    t = g(13) * np.abs(x64).max(1, keepdims=True) * rstd
    return np.concatenate([rstd * (g(16) + t * t), t + np.abs(rstd * mean) * (g(17) + t * t)], axis=1)


def make_parts(x64, nparts):
    """the partial statistics a producer leaves behind: per 64-column part (sum, sum of squares centred on the part's own mean),
    computed in float64 and rounded once -> f32 [M, nparts, 2]"""
    p = np.asarray(x64, dtype=F64)[:, :64 * nparts].reshape(len(x64), nparts, 64)
    s = p.sum(2)
    m2 = ((p - p.mean(2, keepdims=True)) ** 2).sum(2)
    return np.stack([s, m2], axis=2).astype(F)


def parts_ref(parts, eps):
    """Chan's combination in float64 from the float32 parts -> (coef [M, 2], bound [M, 2])"""
    p = np.asarray(parts, dtype=F64)
    nparts = p.shape[1]
    Dn = 64.0 * nparts
    s, m2 = p[..., 0], p[..., 1]
    mean = s.sum(1, keepdims=True) / Dn
    d = s / 64.0 - mean
    M2 = (m2 + 64.0 * d * d).sum(1, keepdims=True)
    rstd = 1.0 / np.sqrt(M2 / Dn + F64(F(eps)))
    coef = np.concatenate([rstd, -rstd * mean], axis=1)
    dm = g(5) * np.abs(s).sum(1, keepdims=True) / Dn
    dM2 = 128.0 * dm * np.abs(d).sum(1, keepdims=True) + 64.0 * nparts * dm * dm + g(7) * M2
    rel = dM2 * rstd * rstd / (2.0 * Dn) + 4 * U
    return coef, np.concatenate([rstd * rel, np.abs(rstd * mean) * (rel + U) + rstd * dm], axis=1)


# ---------------------------------------------------------------------------------------------------------------------------------
# float32 restatements of the LayerNorm group
# ---------------------------------------------------------------------------------------------------------------------------------
def wave_sum(v):
    """the DPP butterfly of common.h over the last axis (64 lanes): lane^1, lane^2, the other quad, the other half row, the other
    row, the other half -- additions commute, so it is the tree of neighbouring pairs"""
    v = np.asarray(v, dtype=F)
    assert v.shape[-1] == 64
    while v.shape[-1] > 1:
        v = v[..., 0::2] + v[..., 1::2]
    return v[..., 0]


def _lanes(x, per):
    """[M, D] -> [M, nv, 64, per] zero-padded, and the mask of the columns that exist"""
    M, D = x.shape
    nv = -(-D // (64 * per))
    pad = np.zeros((M, nv * 64 * per), dtype=F)
    pad[:, :D] = x
    live = np.zeros((M, nv * 64 * per), dtype=bool)
    live[:, :D] = True
    return pad.reshape(M, nv, 64, per), live.reshape(M, nv, 64, per)


def _tree4(a):
    return (a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])


def _tree8(a):
    return ((a[..., 0] + a[..., 1]) + (a[..., 2] + a[..., 3])) + ((a[..., 4] + a[..., 5]) + (a[..., 6] + a[..., 7]))


def emulate_stats(x, eps, per=4, fault=None):
    """(mean, rstd) [M, 1] float32 in the kernels' order: per = 4 columns per lane and group (layernorm_kernel, hilo_rows_kernel),
    per = 8 (ln_coef_kernel: a tree over the 8 for the sum, serial for the squares)"""
    x = np.asarray(x, dtype=F)
    M, D = x.shape
    eps = F(eps)
    Dstat = D
    if fault == "tail_columns_dropped":
        Dstat = 256 * (D // 256)
    v, live = _lanes(x, per)
    if Dstat != D:
        live = live & (np.arange(v[0].size).reshape(v.shape[1:]) < Dstat)[None]
        v = np.where(live, v, F(0))
    width = F(v[0].size) if fault == "divide_by_padded_width" else F(max(Dstat, 1))
    invD = F(1) / width
    s = np.zeros((M, 64), dtype=F)
    for i in range(v.shape[1]):
        s = s + (_tree4(v[:, i]) if per == 4 else _tree8(v[:, i]))
    mean = (wave_sum(s) * invD).reshape(M, 1)
    q = np.zeros((M, 64), dtype=F)
    if fault == "one_pass_variance":
        for i in range(v.shape[1]):
            sq = v[:, i] * v[:, i]
            q = q + (_tree4(sq) if per == 4 else _tree8(sq))
        var = wave_sum(q) * invD - mean[:, 0] * mean[:, 0]
    else:
        for i in range(v.shape[1]):
            a = np.where(live[:, i], v[:, i] - mean[:, :, None], F(0))
            if per == 4:
                q = q + _tree4(a * a)
            else:
                for j in range(8):
                    q = q + a[..., j] * a[..., j]
        var = wave_sum(q) * invD
        if fault == "unbiased_variance":
            var = wave_sum(q) * (F(1) / F(max(D - 1, 1)))
    with np.errstate(all="ignore"):
        if fault == "eps_outside_sqrt":
            rstd = F(1) / (np.sqrt(var) + eps)
        elif fault == "eps_ignored":
            rstd = F(1) / np.sqrt(var + F(1e-5))
        else:
            rstd = F(1) / np.sqrt(var + eps)
    rstd = rstd.astype(F).reshape(M, 1)
    if fault == "stats_from_next_row" and M > 1:
        mean, rstd = np.roll(mean, -1, axis=0), np.roll(rstd, -1, axis=0)
    return mean, rstd


def emulate_layernorm(x, gamma, beta, eps, out="f32", fault=None):
    """layernorm_kernel / hilo_rows_kernel on a float32 row -> f32 [M, D]; out = 'bf16': rounded to bf16; out = 'hilo': (hi, lo)"""
    x = np.asarray(x, dtype=F)
    mean, rstd = emulate_stats(x, eps, 4, fault)
    gamma, beta = np.asarray(gamma, dtype=F), np.asarray(beta, dtype=F)
    if fault == "gamma_shifted_4":
        gamma = np.roll(gamma, -4)
    with np.errstate(all="ignore"):
        y = ((x - mean) * rstd * gamma + beta).astype(F)
    if out == "bf16":
        return bf16_round(y)
    if out == "hilo":
        return split_hilo(y)
    return y


def emulate_hilo_input(hi, lo, shift=None, fault=None):
    """the row as hilo_rows_kernel rebuilds it: fl(hi + lo), then fl(. + shift[row])"""
    hi, lo = np.asarray(hi, dtype=F), np.asarray(lo, dtype=F)
    x = hi if fault == "lo_plane_ignored" else hi + lo
    if shift is not None and fault != "shift_ignored":
        sh = np.asarray(shift, dtype=F)
        if fault == "shift_from_next_row":
            sh = np.roll(sh, -1)
        x = x + sh[:, None]
    return x.astype(F)


def emulate_layernorm_hilo(hi, lo, gamma, beta, eps, out="f32", fault=None):
    hfault = fault if fault in HILO_FAULTS else None
    return emulate_layernorm(emulate_hilo_input(hi, lo, None, hfault), gamma, beta, eps, out, None if hfault else fault)


def emulate_join(hi, lo, fault=None):
    return emulate_hilo_input(hi, lo, None, fault)


def emulate_unshift(hi, lo, shift, fault=None):
    return split_hilo(emulate_hilo_input(hi, lo, shift, fault))


def emulate_ln_coef(hi, eps, fault=None):
    """ln_coef_kernel: the statistics of the hi plane alone -> (rstd, -rstd mean) f32 [M, 2]"""
    mean, rstd = emulate_stats(hi, eps, 8, fault)
    return np.concatenate([rstd, -rstd * mean], axis=1).astype(F)


def emulate_ln_coef_parts(parts, eps, fault=None, return_mean=False):
    """ln_coef_parts_kernel / ln_coef_row, operation for operation (common.h lnp_*).  Without a fault the mean and the argument of
    the square root are the kernel's bits; the square root itself is the hardware's on the GPU (__fsqrt_rn is v_sqrt_f32, one ulp,
    unless the toolchain is told to round it), so rstd may differ from this one by up to 3 ulp: parts_bits_match.
    return_mean: -> (coef, mean [M])"""
    p = np.asarray(parts, dtype=F)
    M, nparts, _ = p.shape
    use = min(nparts, 8) if fault == "upper_parts_dropped" else nparts
    width = F(1024) if fault == "width_taken_as_1024" else F(nparts * 64)
    full = np.zeros((M, 16, 2), dtype=F)
    full[:, :use] = p[:, :use]
    has = np.arange(16) < use

    def tree8(v):
        return ((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])) + ((v[:, 4] + v[:, 5]) + (v[:, 6] + v[:, 7]))

    mean = (tree8(full[:, :8, 0] + full[:, 8:, 0]) / width).astype(F)
    d = (full[..., 0] * F(1.0 / 64.0) - mean[:, None]).astype(F)
    term = full[..., 1] if fault == "part_means_not_recentred" else fmaf((F(64) * d).astype(F), d, full[..., 1])
    term = np.where(has[None], term, F(0)).astype(F)
    m2 = tree8(term[:, :8] + term[:, 8:])
    rstd = (F(1) / np.sqrt((m2 / width).astype(F) + F(eps))).astype(F)
    coef = np.stack([rstd, (-rstd) * mean], axis=1).astype(F)
    return (coef, mean) if return_mean else coef


def parts_bits_match(got, parts, eps):
    """got [M, 2] from the GPU against the restatement: rstd within 3 ulp (a square root that is one ulp off moves 1 / sqrt by at
    most 2^-23 of its value, two ulp, and the division rounds once more), and -rstd mean the float32 product of the rstd that was
    stored and the restatement's mean, bit for bit: the sums ran in the kernel's order.  -> None, or a message"""
    emu, mean = emulate_ln_coef_parts(parts, eps, return_mean=True)
    got = np.asarray(got, dtype=F)
    off = np.abs(got[:, 0].astype(F64) - emu[:, 0].astype(F64)) / np.spacing(emu[:, 0]).astype(F64)
    if not (off <= 3).all():
        r = int(np.argmax(off))
        return f"rstd of row {r} is {off[r]:g} ulp from the restatement: {got[r, 0]!r} != {emu[r, 0]!r}"
    want = ((-got[:, 0]) * mean).astype(F)
    bad = got[:, 1].view(np.uint32) != want.view(np.uint32)
    if bad.any():
        r = int(np.argmax(bad))
        return f"-rstd mean of row {r}: {got[r, 1]!r} != {want[r]!r} = -({got[r, 0]!r}) * {mean[r]!r}"
    return None


# ---------------------------------------------------------------------------------------------------------------------------------
# masked_ce
# ---------------------------------------------------------------------------------------------------------------------------------
CE_FAMILIES = ("base", "plus100", "minus3000", "peaky", "flat", "mixed")
CE_LABEL_COLUMNS = (0, 3, 4, 255, 256, -4, -1)


def ce_labels(M, V, start=0):
    """the columns 0, 3, 4, 255, 256, V - 4, V - 1 that exist, in turn from `start`: all inside [0, V)"""
    cols = [c % V if c < 0 else c for c in CE_LABEL_COLUMNS if (c < 0 or c < V)]
    cols = sorted(set(cols))
    return np.array([cols[(start + r) % len(cols)] for r in range(M)], dtype=np.int64)


def ce_row(kind, V, label, rng):
    base = 4.0 * rng.standard_normal(V)
    if kind == "base":
        return base
    if kind == "plus100":
        return base + 100.0
    if kind == "minus3000":
        return base - 3000.0
    if kind == "peaky":
        x = np.full(V, -60.0)
        x[label] = 60.0
        return x
    if kind == "flat":
        return np.full(V, 2.5)
    raise ValueError(kind)


def ce_family(kind, M, V, seed=0):
    """-> dict(logits f32 [M, V], labels int64 [M], mask f32 [M]); 'mixed': the five kinds row by row.  Every third row from the
    second is not masked (mask 0), unless there is one row only."""
    fi = CE_FAMILIES.index(kind)
    rng = np.random.default_rng(31 * V + 7 * M + fi + seed)
    labels = ce_labels(M, V, start=5 * fi)
    kinds = [CE_FAMILIES[r % 5] if kind == "mixed" else kind for r in range(M)]
    logits = np.stack([ce_row(k, V, int(labels[r]), rng) for r, k in enumerate(kinds)]).astype(F)
    mask = np.ones(M, dtype=F)
    if M > 1:
        mask[1::3] = 0.0
    return dict(logits=logits, labels=labels, mask=mask)


def ce_nv4(V):
    return 1 if V <= 256 else 4 if V <= 1024 else 32 if V <= 8192 else 64


def ce_ref(logits, labels, mask, eps):
    """float64 rows and loss with their bounds -> (rows, row_bound, loss, loss_bound); eps as the kernel gets it (a float)"""
    x = np.asarray(logits, dtype=F64)
    M, V = x.shape
    eps = F64(F(eps))
    m = np.asarray(mask, dtype=F64)
    nv4 = ce_nv4(V)
    mx = x.max(1)
    e = np.exp(x - mx[:, None])
    se = e.sum(1)
    lse = mx + np.log(se)
    xl = x[np.arange(M), np.asarray(labels)]
    nll = lse - xl
    smooth = lse - x.mean(1)
    row = ((1 - eps) * nll + eps * smooth) * m
    w = (e * np.abs(x - mx[:, None])).sum(1) / se
    dlse = g(w + 3 + nv4 + 8) + 2 * U * np.abs(np.log(se)) + U * np.abs(lse)
    dnll = dlse + U * np.abs(nll)
    dsm = dlse + g(nv4 + 10) * np.abs(x).mean(1) + U * np.abs(smooth)
    drow = ((1 - eps) * (dnll + 2 * U * np.abs(nll)) + eps * (dsm + U * np.abs(smooth)) + U * np.abs(row)) * np.abs(m)
    with np.errstate(all="ignore"):
        loss = row.sum() / m.sum()
        dloss = drow.sum() / m.sum() + U * abs(loss)
    return row, drow, loss, dloss


def emulate_masked_ce(logits, labels, mask, eps, fault=None):
    """masked_ce_rows_kernel + masked_ce_reduce_kernel in float32 (np.exp / np.log for the device's) -> (rows f32 [M], loss f32)"""
    x = np.asarray(logits, dtype=F)
    M, V = x.shape
    labels = np.asarray(labels)
    mask = np.asarray(mask, dtype=F)
    eps = F(eps)
    nv4 = ce_nv4(V)
    pad = np.full((M, nv4 * 256), -np.inf, dtype=F)
    pad[:, :V] = x
    v = pad.reshape(M, nv4, 64, 4)
    mx = x.max(1).reshape(M, 1, 1)
    with np.errstate(all="ignore"):
        se = np.zeros((M, 64), dtype=F)
        sx = np.zeros((M, 64), dtype=F)
        for i in range(nv4):
            arg = v[:, i] if fault == "no_max_subtraction" else v[:, i] - mx
            se = se + _tree4(np.exp(arg).astype(F))
            sx = sx + _tree4(np.where(np.isfinite(v[:, i]), v[:, i], F(0)))
        se, sx = wave_sum(se), wave_sum(sx)
        lse = (np.log(se).astype(F) if fault == "no_max_subtraction" else mx[:, 0, 0] + np.log(se).astype(F)).astype(F)
        lab = np.roll(labels, -1) if fault == "label_from_next_row" else labels
        nll = lse - x[np.arange(M), lab]
        width = F(nv4 * 256) if fault == "smoothing_mean_over_padded_width" else F(V)
        smooth = lse - sx / width
        a, b = (eps, F(1) - eps) if fault == "eps_weights_swapped" else (F(1) - eps, eps)
        rows = ((a * nll + b * smooth) * mask).astype(F)
        den = F64(M) if fault == "mean_over_all_rows" else mask.astype(F64).sum()
        loss = F(rows.astype(F64).sum() / den)
    return rows, loss


# ---------------------------------------------------------------------------------------------------------------------------------
# random_mask
# ---------------------------------------------------------------------------------------------------------------------------------
NOISE_KINDS = ("uniform", "all_equal", "heavy_ties", "signed_zeros")


def mask_noise(kind, B, N, seed=0):
    rng = np.random.default_rng(17 * N + B + seed + NOISE_KINDS.index(kind))
    if kind == "uniform":
        return rng.random((B, N)).astype(F)
    if kind == "all_equal":
        return np.full((B, N), 0.25, dtype=F)
    if kind == "heavy_ties":
        return (rng.integers(0, 3, (B, N)) * 0.25).astype(F)
    if kind == "signed_zeros":                                  # -0.0 == +0.0: ties, decided by the index alone
        x = np.where(rng.random((B, N)) < 0.5, -0.0, 0.0).astype(F)
        x[:, ::7] = 0.5
        return x
    raise ValueError(kind)


def mask_family(B, N, E, kind, seed=0):
    rng = np.random.default_rng(5 * N + E + seed)
    z = rng.standard_normal((B, N, E)).astype(F)
    tok = (100.0 + np.arange(E)).astype(F)                      # every column its own value, none of them a value of z
    return dict(z=z, noise=mask_noise(kind, B, N, seed), mask_token=tok)


def mask_ref(z, noise, mask_token, len_keep):
    """oracle.random_masking's rule for a given len_keep: position i is masked iff its rank in a STABLE ascending sort of the noise
    is >= len_keep -> (x [B, N, E], mask [B, N])"""
    order = np.argsort(noise, axis=1, kind="stable")
    rank = np.argsort(order, axis=1, kind="stable")
    mask = (rank >= len_keep).astype(F)
    x = np.where(mask[..., None] > 0, np.asarray(mask_token, dtype=F).reshape(1, 1, -1), np.asarray(z, dtype=F))
    return x.astype(F), mask


def emulate_random_mask(z, noise, mask_token, len_keep, fault=None):
    """random_mask_kernel: every position counts the positions ordered before it (O(N^2): small N only)"""
    z, nz, tok = np.asarray(z, dtype=F), np.asarray(noise, dtype=F), np.asarray(mask_token, dtype=F)
    B, N, E = z.shape
    j, i = np.arange(N)[None, :, None], np.arange(N)[None, None, :]
    o, mine = nz[:, :, None], nz[:, None, :]
    tie = (j > i) if fault == "ties_to_larger_index" else (j < i)
    rank = ((o < mine) | ((o == mine) & tie)).sum(1)
    mask = ((rank > len_keep) if fault == "rank_off_by_one" else (rank >= len_keep)).astype(F)
    fill = tok[np.arange(N) % E][None, :, None] if fault == "token_column_from_row" else tok.reshape(1, 1, E)
    x = np.where(mask[..., None] > 0, np.broadcast_to(fill, z.shape), z)
    return x.astype(F), mask


# ---------------------------------------------------------------------------------------------------------------------------------
# row utilities: exact, numpy indexing
# ---------------------------------------------------------------------------------------------------------------------------------
def patchify_ref(img, P):
    """out[(b, ph, pw), (c, i, j)] = img[b, c, ph P + i, pw P + j]"""
    B, C, H, W = img.shape
    x = img.reshape(B, C, H // P, P, W // P, P).transpose(0, 2, 4, 1, 3, 5)
    return np.ascontiguousarray(x).reshape(B * (H // P) * (W // P), C * P * P)


def unpatchify_ref(y, B, C, H, W, P, lo, hi):
    """img[b, c, ph P + i, pw P + j] = clamp(y[(b, ph, pw), (i P + j) C + c]), NaN kept (torch.clamp)"""
    x = np.asarray(y, dtype=F).reshape(B, H // P, W // P, P, P, C).transpose(0, 5, 1, 3, 2, 4)
    x = np.ascontiguousarray(x).reshape(B, C, H, W)
    with np.errstate(invalid="ignore"):
        return np.where(x < F(lo), F(lo), np.where(x > F(hi), F(hi), x)).astype(F)


def convert_pad_ref(x, Kpad):
    out = np.zeros((x.shape[0], Kpad), dtype=F)
    out[:, :x.shape[1]] = x
    return out


def embed_rows_ref(table, ids, Kpad):
    V, E = table.shape
    rows = np.clip(np.asarray(ids, dtype=np.int64), 0, V - 1)
    return convert_pad_ref(table[rows], Kpad)


def add_rows_ref(x, table):
    return (x + table[np.arange(len(x)) % len(table)]).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------------------
def ratio(got, want, bound):
    """worst |got - want| / bound (inf where got is not finite or the bound is exceeded at a zero bound)"""
    got, want, bound = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64), np.asarray(bound, dtype=F64)
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        r = np.where(err == 0, 0.0, err / bound)
        r = np.where(np.isfinite(got), r, np.inf)
    return float(np.max(r)) if r.size else 0.0


def assert_within(got, want, bound, what, kinds=None):
    got, want, bound = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64), np.asarray(bound, dtype=F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bound = np.broadcast_to(bound, want.shape)
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        bad = ~(err <= bound)
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        kind = f", a {kinds[at[0]]} row" if kinds is not None else ""
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside their bound, the first at {at}{kind}: got {got[at]!r}, "
                             f"wanted {want[at]!r}, |error| {err[at]:.3e} > bound {bound[at]:.3e} (worst ratio {ratio(got, want, bound):.3g})")
    return ratio(got, want, bound)
