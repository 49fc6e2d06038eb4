"""Probes for the vector quantiser (paintmind_amd/csrc/vq.hip): inputs on which a kernel that left the contract's arithmetic order,
its first-minimum rule or its tile and split map would give other token indices, and a numpy restatement of the kernel in which
such faults can be planted one at a time (tests/test_vq_probes_cpu.py proves that each is rejected; tests/test_gpu_vq_probes.py
holds the kernel to the same comparisons).  numpy only: no torch, nothing that needs a GPU; not a conftest, not collected.

The contract (vq.hip's header, restated by oracle/vq_ref.c):
    ss  = fmaf(z[k], z[k], ss)            k ascending, from +0
    zn  = z / fmaxf(sqrtf(ss), 1e-12f)
    sz  = fmaf(zn[k], zn[k], sz)
    dot = fmaf(zn[k], en[j][k], dot)
    d_j = (sz + sq[j]) - 2 dot
    idx = the first j with the smallest d_j
Everything is compared bit for bit, so nothing here has a tolerance.

The kernel's layout, restated for `where` / `row_where` and for `emulate`: V >= 2048 codes are scanned in 4 splits of
cps = ceil(ceil(V / 4) / 128) * 128 codes (fewer: one split); a split goes through LDS in tiles of TC = 128 codes, a tile in 8 groups
of 16 codes, code j in lane j % 16 of a 16-lane DPP row.  Every lane keeps the first minimum over its codes in ascending order
(strict '<'), the 16 lanes are reduced on (distance, index), and a finishing kernel merges the splits in ascending order with a
strict '<'.  A workgroup owns 256 rows, a wave 64 of them; row 16 rt + 4 g + r of a wave is accumulator register r of lane group g in
row tile rt.  Codes past the split's end in its last tile are loaded as en = 0, sq = +inf: their distance is +inf and never wins.
"""
import numpy as np

F = np.float32
F64 = np.float64
TC = 128
WIDTHS = (8, 16, 32, 64)
ULP = 2.0 ** -22                 # of a distance's larger operand: sz + sq is 2 up to rounding, and the spacing of floats in [2, 4) is 2^-22
FAULTS = ("dot_descending_k", "dot_unfused", "dist_reassociated", "last_minimum", "lane_tie_keeps_lower_lane",
          "lane_tie_takes_other_lane", "split_merge_keeps_later", "pad_codes_are_zero", "split_short_by_one_tile", "clamp_dropped",
          "flush_subnormals")


# ---------------------------------------------------------------------------------------------------------------------------------
# geometry
# ---------------------------------------------------------------------------------------------------------------------------------
def vq_splits(V):
    return 4 if V >= 2048 else 1


def cps(V):
    """codes per split"""
    per = -(-V // vq_splits(V))
    return -(-per // TC) * TC


def split_ranges(V):
    c = cps(V)
    return [(s * c, min(V, (s + 1) * c)) for s in range(vq_splits(V))]


def where(j, V):
    """code index -> (split, tile of the split, 16-code group of the tile, lane)"""
    c = cps(V)
    s, off = int(j) // c, int(j) % c
    return s, off // TC, off % TC // 16, int(j) % 16


def row_where(m):
    """row index -> (block, wave, row tile, g, r): row = 256 block + 64 wave + 16 rt + 4 g + r"""
    m = int(m)
    return m // 256, m % 256 // 64, m % 64 // 16, m % 16 // 4, m % 4


def _code_text(j, V):
    if not 0 <= j < V:
        return f"{j} (NOT a code: V = {V}; it would sit at split {where(j, V)[0]}, tile {where(j, V)[1]}, group {where(j, V)[2]}, lane {where(j, V)[3]})"
    s, tile, grp, lane = where(j, V)
    return f"{j} (split {s}, tile {tile}, group {grp}, lane {lane})"


def describe(row, got, want, V, gap=None):
    b, w, rt, g, r = row_where(row)
    text = (f"row {row} (block {b}, wave {w}, row tile {rt}, g {g}, r {r}): got code {_code_text(int(got), V)}, "
            f"wanted {_code_text(int(want), V)}")
    if gap is not None:
        text += f"; the oracle's best-to-second gap of this row is {float(gap):.3e} = {float(gap) / ULP:g} ulp"
    return text


def assert_idx(got, want, V, gap=None, what="idx", rows=None):
    """idx equal everywhere (on `rows` if given: a boolean mask or an index array); the message names the first three rows"""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    if rows is not None:
        keep = np.zeros(len(got), dtype=bool)
        keep[rows] = True
        bad &= keep
    if bad.any():
        first = np.nonzero(bad)[0][:3]
        lines = [describe(m, got[m], want[m], V, None if gap is None else gap[m]) for m in first]
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(got)} indices differ (V = {V}, {vq_splits(V)} split(s) of {cps(V)} codes)\n  "
                             + "\n  ".join(lines))


def bits(a):
    """float32 array -> uint32 view (bit-for-bit comparisons: -0.0 != 0.0, NaN == NaN)"""
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def assert_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        at = tuple(int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in their bits, the first at {at}: "
                             f"{got[at]!r} (0x{int(bits(got)[at]):08x}) != {want[at]!r} (0x{int(bits(want)[at]):08x})")


# ---------------------------------------------------------------------------------------------------------------------------------
# fmaf in numpy
# ---------------------------------------------------------------------------------------------------------------------------------
def _fmaf_odd(a, b, c):
    """exact fmaf, element by element: the float64 sum of the (exact) float64 product and c, rounded TO ODD (its error term is
    known exactly, Knuth's two-sum), then to float32.  53 >= 2 * 24 + 2 bits: the second rounding sees what an infinitely precise
    sum would show it."""
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    raw = s.view(np.int64)
    fix = (err != 0) & ((raw & 1) == 0)
    away = (err > 0) == (s > 0)
    raw = np.where(fix, raw + np.where(away, 1, -1), raw)
    return raw.view(F64).astype(F)


def fmaf(a, b, c):
    """float32 fmaf(a, b, c) with ONE rounding.  The float64 product is exact and the float64 sum is rounded once more when it is
    cast to float32; the two roundings differ from one only if the float64 sum lands exactly on the midpoint of two floats (low 29
    bits 0x10000000), or in the subnormal range where the midpoints lie elsewhere: those elements are redone by _fmaf_odd."""
    with np.errstate(all="ignore"):
        s = a.astype(F64) * b
        s = s + c
        r = s.astype(F)
        risky = ((s.view(np.int64) & 0x1FFFFFFF) == 0x10000000) | ((np.abs(s) < 2.0 ** -126) & (s != 0))
        if risky.any():
            a, b, c = (np.broadcast_to(np.asarray(x, dtype=F), s.shape) for x in (a, b, c))
            r[risky] = _fmaf_odd(a[risky], b[risky], c[risky])
    return r


def _ftz(x):
    return np.where(np.abs(x) < F(2.0 ** -126), np.copysign(F(0), x), x).astype(F)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel in numpy, with one fault at a time
# ---------------------------------------------------------------------------------------------------------------------------------
def normalize(x, fault=None):
    """rows of x -> (x / max(|x|, 1e-12), sum of its squares), in the contract's order"""
    x = np.ascontiguousarray(x, dtype=F)
    M, E = x.shape
    with np.errstate(all="ignore"):
        ss = np.zeros(M, dtype=F)
        for k in range(E):
            ss = fmaf(x[:, k], x[:, k], ss)
        den = np.sqrt(ss)
        if fault != "clamp_dropped":
            den = np.maximum(den, F(1e-12))
        xn = (x / den[:, None]).astype(F)
        if fault == "flush_subnormals":
            xn = _ftz(xn)
        s2 = np.zeros(M, dtype=F)
        for k in range(E):
            s2 = fmaf(xn[:, k], xn[:, k], s2)
    return xn, s2


def _distances(zn, sz, en, sq, fault):
    E = zn.shape[1]
    enT = np.ascontiguousarray(en.T)
    dot = np.zeros((zn.shape[0], en.shape[0]), dtype=F)
    with np.errstate(all="ignore"):
        for k in (range(E - 1, -1, -1) if fault == "dot_descending_k" else range(E)):
            if fault == "dot_unfused":
                dot = zn[:, k:k + 1] * enT[k][None, :] + dot                  # float32 product, float32 sum: two roundings
            else:
                dot = fmaf(zn[:, k:k + 1], enT[k][None, :], dot)
            if fault == "flush_subnormals":
                dot = _ftz(dot)
        if fault == "dist_reassociated":
            return sz[:, None] + (sq[None, :] - F(2) * dot)
        return (sz[:, None] + sq[None, :]) - F(2) * dot


_LANES = np.arange(16)
# row_min_step's four DPP controls: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
_BUTTERFLY = (_LANES ^ 1, _LANES ^ 2, (_LANES & 8) | (7 - (_LANES & 7)), 15 - _LANES)


def _scan(d, sz, V, fault):
    """distances [m, V] -> (best distance, index) per row through the kernel's structure: lanes, 16-lane reduction, split merge"""
    m = d.shape[0]
    d = np.where(np.isnan(d), F(np.inf), d)                  # a NaN distance is never '<' anything: the lane keeps what it has
    ranges = split_ranges(V)
    best_d = best_i = None
    for v0, v1 in ranges:
        nt = -(-(v1 - v0) // TC)
        if fault == "split_short_by_one_tile" and len(ranges) > 1:
            nt -= 1
        width = nt * TC
        real = min(width, v1 - v0)
        tile = np.full((m, width), F(np.inf), dtype=F)       # codes past the split's end: sq = +inf
        if fault == "pad_codes_are_zero":
            tile[:] = sz[:, None]                            # en = 0, sq = 0: (sz + 0) - 2 * 0
        tile[:, :real] = d[:, v0:v0 + real]
        lanes = tile.reshape(m, nt * (TC // 16), 16)
        if nt == 0:
            ld, li = np.full((m, 16), F(np.inf), dtype=F), np.full((m, 16), v0, dtype=np.int64)
        else:
            if fault == "last_minimum":                      # '<=' in the lane's scan
                pos = lanes.shape[1] - 1 - np.argmin(lanes[:, ::-1, :], axis=1)
            else:
                pos = np.argmin(lanes, axis=1)               # first occurrence
            ld = np.take_along_axis(lanes, pos[:, None, :], axis=1)[:, 0, :]
            li = v0 + pos * 16 + _LANES[None, :]
            if fault != "last_minimum":
                li = np.where(ld < F(np.inf), li, v0)        # nothing was below the initial +inf: the initial index stays
        for perm in _BUTTERFLY:
            od, oi = ld[:, perm], li[:, perm]
            if fault == "lane_tie_keeps_lower_lane":         # the index is ignored: a lane keeps its own on equal distances
                take = od < ld
            elif fault == "lane_tie_takes_other_lane":       # ... or takes the other lane's
                take = od <= ld
            else:
                take = (od < ld) | ((od == ld) & (oi < li))
            ld, li = np.where(take, od, ld), np.where(take, oi, li)
        sd, si = ld[:, 0], li[:, 0]                          # lane 0 of the DPP row stores
        if best_d is None:
            best_d, best_i = sd, si
        else:
            take = (sd <= best_d) if fault == "split_merge_keeps_later" else (sd < best_d)
            best_d, best_i = np.where(take, sd, best_d), np.where(take, si, best_i)
    return best_d, best_i


def emulate(z, cb, fault=None, beta=0.25):
    """The quantiser as vq.hip computes it -> dict(en, sq, zn, sz, idx, dmin, z_out, sqerr, loss).  sqerr [M] is the row's sum of
    (zq - zn)^2 in float64 and loss = (1 + beta) * mean: the kernel's own summation order is not part of the contract."""
    assert fault is None or fault in FAULTS, fault
    z, cb = np.ascontiguousarray(z, dtype=F), np.ascontiguousarray(cb, dtype=F)
    (M, E), V = z.shape, cb.shape[0]
    en, sq = normalize(cb, fault)
    zn, sz = normalize(z, fault)
    idx, dmin = np.empty(M, dtype=np.int64), np.empty(M, dtype=F)
    step = max(1, 250_000 // V)                              # row chunks that stay in the cache
    for m0 in range(0, M, step):
        rows = slice(m0, m0 + step)
        dmin[rows], idx[rows] = _scan(_distances(zn[rows], sz[rows], en, sq, fault), sz[rows], V, fault)
    with np.errstate(all="ignore"):
        zq = np.where((idx < V)[:, None], en[np.minimum(idx, V - 1)], F(0))       # a faulty index past the codebook reads nothing
        z_out = zn + (zq - zn)
        sqerr = ((zq.astype(F64) - zn.astype(F64)) ** 2).sum(1)
    return dict(en=en, sq=sq, zn=zn, sz=sz, idx=idx, dmin=dmin, z_out=z_out, sqerr=sqerr, loss=(1.0 + beta) * sqerr.sum() / (M * E))


# ---------------------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------------------
def _rng(tag, *key):
    return np.random.default_rng([sum(ord(c) << (8 * i) for i, c in enumerate(tag[:7]))] + [int(k) for k in key])


def _pow2(e):
    return np.ldexp(F(1), np.asarray(e)).astype(F)


def iid(M, V, E, seed=0):
    """the family of tests/test_gpu_ops.py::test_vq_bit_exact_against_c_oracle: an i.i.d. normal codebook, 0.3 * normal queries"""
    rng = _rng("iid", seed, M, V, E)
    return dict(cb=rng.standard_normal((V, E)).astype(F), z=(0.3 * rng.standard_normal((M, E))).astype(F), expect=None)


def near_tie(E, V, M=600, seed=0):
    """Clusters of about 96 codes within 2^-12 of a common direction, queries around the same directions: after normalisation the
    candidates' distances are a few ulp apart or equal, so the index depends on every rounding of the chain and on the first-minimum
    rule.  Rows are scaled by powers of two, which normalisation undoes exactly."""
    rng = _rng("near_tie", seed, E, V, M)
    ncl = max(1, V // 96)
    base = rng.standard_normal((ncl, E))
    cb = base[rng.integers(0, ncl, V)] + 2.0 ** -12 * rng.standard_normal((V, E))
    z = base[rng.integers(0, ncl, M)] + 2.0 ** -12 * rng.standard_normal((M, E))
    cb = cb.astype(F) * _pow2(rng.integers(-3, 4, (V, 1)))
    z = z.astype(F) * _pow2(rng.integers(-3, 4, (M, 1)))
    return dict(cb=cb, z=z, expect=None)


def copy_sets(V):
    """the bitwise copies `duplicates` plants: [(kind, codes)], codes ascending, no code in two sets, an odd number of sets.  What
    does not fit below V, or would reuse a code, is left out."""
    c, S = cps(V), vq_splits(V)
    wanted = [("adjacent_lanes", (19, 20)),                       # (j, j + 1) in one group
              ("group_ends", (32, 47)),                           # (j, j + 15): lanes 0 and 15 of one group
              ("same_lane_next_group", (55, 71)),                 # (j, j + 16)
              ("higher_lane_earlier_group", (85, 96)),            # (16 a + 5, 16 a + 16): the smaller index in the higher lane
              ("same_lane_next_tile", (165, 165 + TC)),           # (j, j + 128)
              ("first_last", (0, V - 1)),
              ("tile_edge", (TC - 1, TC))]
    for s in range(1, S):
        wanted.append((f"split_edge_{s}", (s * c - 1, s * c)))
        wanted.append((f"same_offset_next_split_{s}", ((s - 1) * c + 100 + s, s * c + 100 + s)))
    if S >= 3:
        wanted.append(("three_splits", (110, 110 + c, 110 + 2 * c)))
    wanted.append(("adjacent_lanes_again", (35, 36)))             # only taken to make the count odd
    sets, used = [], set()
    for kind, codes in wanted:
        if kind == "adjacent_lanes_again" and len(sets) % 2 == 1:
            continue
        if max(codes) < V and len(set(codes)) == len(codes) and not used & set(codes):
            sets.append((kind, tuple(codes)))
            used |= set(codes)
    assert len(sets) % 2 == 1, (V, sets)
    return sets


def first_equal_row(cb):
    """for every codebook row the smallest index of a row that is bitwise equal to it"""
    raw = bits(cb)
    _, first, inverse = np.unique(raw, axis=0, return_index=True, return_inverse=True)
    return first[inverse.reshape(-1)].astype(np.int64)


def duplicates(E, V, seed=0):
    """A normal codebook with the bitwise copies of copy_sets(V); query i is 2^s times the source of set i % n_sets, so zn equals
    en of every copy bit for bit: the distance is exactly 0 at every copy and positive elsewhere, and the first minimum is the smallest
    index among the copies -- read off the finished codebook, not off the list of sets."""
    rng = _rng("duplicates", seed, E, V)
    cb = rng.standard_normal((V, E)).astype(F)
    sets = copy_sets(V)
    for _, codes in sets:
        cb[list(codes[1:])] = cb[codes[0]]
    first = first_equal_row(cb)
    n_sets = len(sets)
    M = 64 * n_sets + 5
    i = np.arange(M)
    src = np.array([codes[0] for _, codes in sets])[i % n_sets]
    z = cb[src] * _pow2((i // n_sets) % 7 - 3)[:, None]
    return dict(cb=cb, z=z, expect=first[src], sets=sets, src=src)


def identity(E, V, seed=0):
    """every code of a `duplicates` codebook is asked for once: a missed tile, a missed split or a wrong index offset shows"""
    cb = duplicates(E, V, seed)["cb"]
    j = np.arange(V)
    return dict(cb=cb, z=cb * _pow2(j % 7 - 3)[:, None], expect=first_equal_row(cb))


def antipodal(E, V, seed=0):
    """z = -cb[j]: the best real distance of the single-code case is 4, so whatever a padded code scores, it wins if it takes part"""
    cb = _rng("antipodal", seed, E, V).standard_normal((V, E)).astype(F)
    return dict(cb=cb, z=-cb, expect=None)


DEGENERATE_CODES = dict(zero=3, tiny=10, underflow=20, overflow=30, spread=40)


def spread_row(E):
    """components +-2^(-s k): 1 down to below the smallest normal float, so that the normalised row has subnormal components.
    s = 4.5 where E - 1 steps of it reach 2^-126 (E >= 32), else as large as that takes."""
    s = max(4.5, 135.0 / (E - 1))
    k = np.arange(E)
    with np.errstate(under="ignore"):
        return (np.where(k % 3 == 1, -1.0, 1.0) * 2.0 ** (-s * k)).astype(F)


def degenerate(E, V=300, seed=0):
    """Zero rows, rows whose squared norm underflows (2^-80), is subnormal (2^-70: the 1e-12 clamp decides both) or overflows
    (2^70: zn = +-0), one-hot rows and rows with subnormal normalised components, among ordinary ones.  No NaN, no inf.  Code `spread`
    is 4 times the spread query: en of it equals zn of the query bit for bit, subnormals included, and z_out shows them."""
    rng = _rng("degenerate", seed, E, V)
    cb = rng.standard_normal((V, E)).astype(F)
    D = DEGENERATE_CODES
    cb[D["zero"]] = 0
    cb[D["tiny"]] *= F(2.0 ** -70)
    cb[D["underflow"]] *= F(2.0 ** -80)
    cb[D["overflow"]] *= F(2.0 ** 70)
    sp = spread_row(E)
    cb[D["spread"]] = F(4) * sp
    q = rng.standard_normal((6, E)).astype(F)
    onehot = np.eye(E, dtype=F) * np.where(np.arange(E) % 2 == 0, F(1), F(-1))[:, None]
    z = np.concatenate([np.zeros((1, E), dtype=F), q[0:1] * F(2.0 ** -70), q[1:2] * F(2.0 ** -80), q[2:3] * F(2.0 ** 70),
                        cb[[D["tiny"], D["underflow"], D["overflow"]]], onehot, sp[None], -sp[None], q[3:]])
    assert np.isfinite(cb).all() and np.isfinite(z).all()
    zn, _ = normalize(sp[None])
    tiny = (zn != 0) & (np.abs(zn) < F(2.0 ** -126))
    assert tiny.any(), "the spread row must have a subnormal normalised component"
    return dict(cb=cb, z=z, expect=None, spread_rows=(7 + E, 8 + E))


FAMILIES = dict(near_tie=near_tie, duplicates=duplicates, identity=identity, antipodal=antipodal, degenerate=degenerate)

# (family, E, V, M or None = as the family builds it): what tests/test_gpu_vq_probes.py launches
GPU_CASES = ([("near_tie", E, V, 600) for E in WIDTHS for V in (1000, 2048, 2304)]
             + [("near_tie", 32, V, 600) for V in (2047, 2049)]
             + [("duplicates", E, V, None) for E in WIDTHS for V in (2304, 129)]
             + [("identity", E, V, None) for E in (16, 64) for V in (2049, 2304)]
             + [("antipodal", E, V, None) for E in (8, 32) for V in (1, 17)]
             + [("degenerate", E, 300, None) for E in WIDTHS])
RAGGED_M = (1, 63, 64, 65, 255, 257)             # near_tie at (E, V) = (32, 1000)


def case_id(case):
    name, E, V, M = case
    return f"{name}-E{E}-V{V}" + (f"-M{M}" if M is not None else "")


def build(case):
    """-> the family's dict (cb, z, expect or None, ...), arrays read-only"""
    name, E, V, M = case
    fam = near_tie(E, V, M) if name == "near_tie" else FAMILIES[name](E, V)
    for x in fam.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return fam


def near_tie_shares(gap):
    """-> (share of rows with gap == 0, share with gap <= 2 ulp)"""
    gap = np.asarray(gap)
    return float(np.mean(gap == 0)), float(np.mean(gap <= F(2 * ULP)))
