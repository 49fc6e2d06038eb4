"""Probes for the GEMMs that carry a folded LayerNorm (pmhip_gemm_ln, pmhip_gemm_softmax_stats, pmhip_gemm_heads_ln,
pmhip_gemm_swiglu_ln): a float64 reference built from exactly what the kernel is given, element-wise bounds that are derived
from the arithmetic (not tuned), two input families, and a numpy restatement of the folded epilogue that can be made wrong on
purpose.

No GPU and no torch in here: tests/test_fold_probes_cpu.py proves on the CPU that the probes reject a coefficient taken from
the wrong row, the wrong half of a 256-row tile, the previous tile of a persistent workgroup or the wrong column;
tests/test_gpu_fold_probes.py holds the four kernel routes to the same checks.

A call is a dict: h [M, K] the bf16 hi plane, wg [N, K] the bf16 gamma-scaled weights (both as float32 arrays of bf16 values),
coef [M, 2] = (a_r, b_r), c [N], d [N], bias [N] or None (all float32), plus what the epilogue needs (heads, tokens, q_scale).
The folded epilogue computes   pre[r, n] = a_r * (h_r . wg_n) + b_r * c_n + d_n + bias_n   and then
    'plain'   stores pre as float32                                                    out [M, N]
    'heads'   N = 3 * heads * 64 columns q | k | v; q is multiplied by q_scale; bf16      out [M, N]   (*)
    'swiglu'  N = 2 * Hp packed columns (packing.pack_w12: 16 x1 | 16 x2 | 16 x1 | ...); silu(x1) * x2 in bf16   out [M, Hp]
(*) the kernel stores Q [B, heads, tokens, 64], K [B, heads, tokens, 64] and V^T [B, heads, 64, tokens]; heads_to_flat brings
the three back to the [M, N] matrix, so that a wrong element is named by its GEMM row and column.
"""
import numpy as np

from attention_probes import EPS, U, bf16_round, is_bf16      # noqa: F401  (re-exported: the same constants as the attention probes)

LOG2E = 1.4426950408889634
EPILOGUES = ("plain", "heads", "swiglu")

# kernel selection, restated from dispatch() (csrc/gemm.hip) and launch256() (csrc/gemm256.hip); T256 = (M / 256) * (N / 256)
DEEP128_MAX_T256 = 64         # deep128(): at most 256 tiles of 128x128 (and K >= 256) -> the four-stage 128x128 kernel (route A)
FOLD_SMALL_MAX_T256 = 128     # fold_small(): up to here the 128x128 kernel serves the fold (route B where A does not)
PERSIST256 = 256              # launch256(): more tiles than this -> 256 persistent workgroups walk the tiles (route D), else C
CHUNK128, CHUNK256 = 8, 6     # widths of the L2-aware tile walk (tile_of_block) in the two kernels

# The smallest shapes that reach each route, (M, N, K) per (route, epilogue).  They follow the three thresholds above -- deep128()
# and fold_small() in csrc/gemm.hip, the persistent grid of launch256() in csrc/gemm256.hip: a change of one of them needs a
# change here (tests/test_fold_probes_cpu.py::test_shapes_reach_their_routes fails until then).  heads: 8 heads, q | k | v,
# N = 1536, 256 tokens per image; swiglu: Hp = 1024, N = 2048.  Route D: 272 / 258 / 264 tiles, so 16 / 2 / 8 workgroups walk two.
SHAPES = {
    ("A", "plain"): [(512, 512, 256), (512, 512, 1024)], ("A", "heads"): [(512, 1536, 256)], ("A", "swiglu"): [(512, 2048, 256)],
    ("B", "plain"): [(256, 256, 128), (2304, 2048, 256)], ("B", "heads"): [(256, 1536, 128)], ("B", "swiglu"): [(256, 2048, 128)],
    ("C", "plain"): [(2816, 3072, 128)], ("C", "heads"): [(5632, 1536, 128)], ("C", "swiglu"): [(4352, 2048, 384)],
    ("D", "plain"): [(4352, 4096, 128), (4352, 4096, 384)], ("D", "heads"): [(11008, 1536, 128)], ("D", "swiglu"): [(8448, 2048, 384)],
}
HEADS, TOKENS, Q_SCALE = 8, 256, 0.125

ROW_FAULTS = ("next_row_coef", "group_first_row_coef", "other_half_coef", "previous_tile_coef", "coef_from_previous_call")
COL_FAULTS = ("next_col_cd", "col_plus_4_cd", "col_plus_16_cd", "col_plus_64_cd", "swap_c_d")
FAULTS = ROW_FAULTS + COL_FAULTS + ("drop_bias",)
_COL_SHIFT = {"next_col_cd": 1, "col_plus_4_cd": 4, "col_plus_16_cd": 16, "col_plus_64_cd": 64}


# ---------------------------------------------------------------------------------------------------------------- geometry

def route_of(M, N, K):
    t256 = (M // 256) * (N // 256)
    if t256 <= DEEP128_MAX_T256 and K >= 256:
        return "A"
    if t256 <= FOLD_SMALL_MAX_T256:
        return "B"
    return "C" if t256 <= PERSIST256 else "D"


def _xcd_remap(bid, nblocks):
    q, r = nblocks >> 3, nblocks & 7
    xcd, local = bid & 7, bid >> 3
    return np.where(xcd < r, xcd * (q + 1), r * (q + 1) + (xcd - r) * q) + local


def _tile_of_block(vb, tiles_m, tiles_n, max_chunk):
    nchunks = -(-tiles_n // max_chunk)
    cw = -(-tiles_n // nchunks)
    chunk = vb // (tiles_m * cw)
    cw_here = np.minimum(cw, tiles_n - chunk * cw)
    rem = vb - chunk * tiles_m * cw
    return rem // cw_here, chunk * cw + rem % cw_here


class Walk:
    """Which workgroup computes which tile, and as which tile of its walk (gemm_common.h xcd_remap / tile_of_block, restated).
    tile: edge of the square tile; grid: workgroups launched -- workgroup w computes launch indices w, w + grid, ...
    order[tm, tn] = launch index of the tile; step = order // grid is the tile's place in its workgroup's walk."""

    def __init__(self, M, N, tile, chunk, grid=None, route="?"):
        self.M, self.N, self.tile, self.route = M, N, tile, route
        self.tiles_m, self.tiles_n = -(-M // tile), -(-N // tile)
        nt = self.tiles_m * self.tiles_n
        self.grid = nt if grid is None else min(grid, nt)
        idx = np.arange(nt)
        tm, tn = _tile_of_block(_xcd_remap(idx, nt), self.tiles_m, self.tiles_n, chunk)
        self.order = np.full((self.tiles_m, self.tiles_n), -1, np.int64)
        self.order[tm, tn] = idx
        assert (self.order >= 0).all(), "the tile walk is not a bijection"
        self.tm, self.tn = tm, tn                                   # launch index -> tile

    def step(self):
        return self.order // self.grid

    def previous_m(self):
        """[tiles_m, tiles_n]: tile row of the tile the same workgroup ran before this one (its own where it is the first)"""
        prev = np.where(self.order >= self.grid, self.order - self.grid, self.order)
        return self.tm[prev]

    def describe(self, r, n):
        tm, tn = r // self.tile, n // self.tile
        o = int(self.order[tm, tn])
        return (f"route {self.route}, {self.tile}x{self.tile} tile (m, n) = ({tm}, {tn}), launch index {o}: tile {o // self.grid} of the "
                f"walk of workgroup {o % self.grid} (grid {self.grid})")


def walk_of(M, N, K):
    """the walk of the kernel that dispatch() gives this folded shape"""
    r = route_of(M, N, K)
    if r in "AB":
        return Walk(M, N, 128, CHUNK128, None, r)
    return Walk(M, N, 256, CHUNK256, PERSIST256, r)


# ---------------------------------------------------------------------------------------------------------------- layouts

def swiglu_cols(Hp):
    """(x1 column, x2 column) of the packed GEMM for every hidden column (packing.pack_w12: groups of 16 rows interleaved)"""
    j = np.arange(Hp)
    x1 = (j // 16) * 32 + j % 16
    return x1, x1 + 16


def heads_to_flat(q, k, vt):
    """Q [B, H, t, 64], K [B, H, t, 64], V^T [B, H, 64, t] -> [B * t, 3 * H * 64]"""
    B, H, T, _ = q.shape
    f = lambda x: np.ascontiguousarray(np.transpose(x, (0, 2, 1, 3))).reshape(B * T, H * 64)
    return np.concatenate([f(q), f(k), f(np.transpose(vt, (0, 1, 3, 2)))], axis=1)


def flat_to_heads(x, heads, tokens):
    """inverse of heads_to_flat (tokens a multiple of 64: no padding)"""
    M, N = x.shape
    p = x.reshape(M // tokens, tokens, 3, heads, 64)
    return (np.transpose(p[:, :, 0], (0, 2, 1, 3)), np.transpose(p[:, :, 1], (0, 2, 1, 3)), np.transpose(p[:, :, 2], (0, 2, 3, 1)))


# ---------------------------------------------------------------------------------------------------------------- reference and bound

def _silu(x):
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def reference(call, epilogue):
    """float64 reference and the element-wise bound B on |out - ref|, both in the epilogue's output shape.

    pre = a_r acc + b_r c_n + d_n + bias_n with acc = h_r . wg_n; S[r, n] = sum_k |h_rk| |wg_nk|.  Per f32 operation EPS = 2^-23
    (MFMA accumulation is not guaranteed to round to nearest), per bf16 rounding U = 2^-8.

      f32 result    B = |a_r| (K + 8) EPS S  +  4 EPS (|a_r acc| + |b_r c_n| + |d_n| + |bias_n|)
                    first term: the K-term accumulation of acc (every partial sum is at most S), carried through the multiplication
                    by a_r; second term: ln_apply4's two fused multiply-adds and the bias add, three roundings of values that are at
                    most the sum of the four magnitudes, with one EPS to spare
      heads         K, V: B + U |ref| (one output rounding);  Q: q_scale B + (U + EPS) |ref| (the scale is one more f32 operation)
      swiglu        x1, x2 carry B1, B2; |silu'| <= 1.1, and the gate, the product and the rounding are relative to the result:
                    B = 1.1 B1 |x2| + |silu(x1)| B2 + (U + 8 EPS) |ref|
    """
    h, wg = np.asarray(call["h"], np.float64), np.asarray(call["wg"], np.float64)
    a, b = (np.asarray(call["coef"], np.float64)[:, i][:, None] for i in (0, 1))
    c, d = np.asarray(call["c"], np.float64)[None, :], np.asarray(call["d"], np.float64)[None, :]
    bias = np.zeros_like(c) if call.get("bias") is None else np.asarray(call["bias"], np.float64)[None, :]
    K = h.shape[1]
    acc = h @ wg.T
    S = np.abs(h) @ np.abs(wg).T
    pre = a * acc + b * c + d + bias
    B = np.abs(a) * ((K + 8) * EPS) * S + 4 * EPS * (np.abs(a * acc) + np.abs(b * c) + np.abs(d) + np.abs(bias))
    del acc, S
    if epilogue == "plain":
        return pre, B
    if epilogue == "heads":
        inner = call["heads"] * 64
        qs = float(call["q_scale"])
        pre[:, :inner] *= qs
        B[:, :inner] *= abs(qs)
        B += U * np.abs(pre)
        B[:, :inner] += EPS * np.abs(pre[:, :inner])
        return pre, B
    if epilogue == "swiglu":
        i1, i2 = swiglu_cols(pre.shape[1] // 2)
        x1, x2, B1, B2 = pre[:, i1], pre[:, i2], B[:, i1], B[:, i2]
        s = _silu(x1)
        ref = s * x2
        return ref, 1.1 * B1 * np.abs(x2) + np.abs(s) * B2 + (U + 8 * EPS) * np.abs(ref)
    raise ValueError(epilogue)


def gemm_col(epilogue, n):
    """GEMM column behind output column n (SwiGLU: the x1 column; x2 is 16 further)"""
    return int((n // 16) * 32 + n % 16) if epilogue == "swiglu" else int(n)


def worst_ratio(out, ref, B):
    """max over elements of err / B (0 / 0 = 0; anything non-finite, or err > 0 = B, -> inf) and its (row, column)"""
    o = np.asarray(out, np.float64)
    err = np.abs(o - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / B)
    ratio = np.where(np.isfinite(o), ratio, np.inf)
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    idx = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[idx]), (int(idx[0]), int(idx[1]))


def check_bound(out, ref, B, call, epilogue, walk, what=""):
    """-> (largest err / B, None), or (largest, message naming the worst (row, column), its route and tile and the row's (a_r, b_r))"""
    ratio, (r, n) = worst_ratio(out, ref, B)
    if ratio <= 1.0:
        return ratio, None
    a, b = (float(x) for x in np.asarray(call["coef"])[r])
    return ratio, (f"{what}: |out - ref| exceeds the bound at (row, column) = ({r}, {n}): out {float(np.asarray(out)[r, n])!r} ref {ref[r, n]!r} "
                   f"bound {B[r, n]!r} err / B = {ratio:.3g}; {walk.describe(r, gemm_col(epilogue, n))}; (a_r, b_r) = ({a!r}, {b!r})")


def first_difference(out, want, epilogue, walk, what=""):
    """None where out == want everywhere, else a message naming the first wrong (row, column) and its tile"""
    bad = np.asarray(out) != np.asarray(want)
    if not bad.any():
        return None
    r, n = (int(x) for x in np.argwhere(bad)[0])
    rows = int(bad.any(1).sum())
    return (f"{what}: {int(bad.sum())} elements in {rows} rows differ; first (row, column) = ({r}, {n}): got {float(np.asarray(out)[r, n])!r} want "
            f"{float(np.asarray(want)[r, n])!r}; {walk.describe(r, gemm_col(epilogue, n))}")


# ---------------------------------------------------------------------------------------------------------------- families

def _code(idx):
    """idx 0..511 -> 512 distinct dyadic values with 8 significant bits: +-(129 + m) / 128 * 2^e, m < 128, e in {0, 1}: magnitudes
    in (1, 4], never 0 or 1; bit 8 of idx is the sign"""
    idx = np.asarray(idx, np.int64)
    mag = (129 + (idx & 127)) / 128.0 * (1 + ((idx >> 7) & 1))
    return np.where((idx >> 8) & 1, -mag, mag).astype(np.float32)


def row_code(r, which=0, signed=True):
    """The code of a row.  The MAGNITUDE alone (256 values) already differs between rows 1 .. 255 apart inside a 256-row tile,
    between rows 1, 4, 8, 16, 64 and 128 apart across a tile edge, and between rows 256 * k apart for every k < 256 (37, 91 and
    101, 57 are odd).  which = 0: b_r; 1: a_r; 2, 3: the coefficients of 'another call'."""
    r = np.asarray(r, np.int64)
    mul, tmul, off = ((37, 101, 0), (91, 57, 13), (37, 101, 77), (91, 57, 150))[which]
    idx = (mul * (r % 256) + tmul * (r // 256) + off) % 256
    sign = ((r * 7 + (r >> 3) + (r >> 8) + which) & 1) if signed else 0
    return _code(idx + 256 * sign)


def _col_kind(n):
    """True = c-column, False = d-column: alternates inside a lane's 4 columns and flips under a shift of the column by 1, 4, 16 or
    64 in three columns of four"""
    n = np.asarray(n, np.int64)
    return ((n ^ (n >> 2) ^ (n >> 4) ^ (n >> 6)) & 1) == 0


def _pow2_col(n, e0, ne):
    """+-2^e per column, e in [e0, e0 + ne)"""
    n = np.asarray(n, np.int64)
    e = e0 + (5 * n + 3 * (n >> 2) + (n >> 4) + (n >> 6)) % ne
    sign = ((n >> 1) ^ (n >> 3) ^ (n >> 5) ^ (n >> 7)) & 1
    return np.where(sign, -1.0, 1.0) * np.exp2(e)


def index_call(epilogue, M, N, K, variant=0, heads=8, tokens=256, q_scale=0.125):
    """The `index` family: an all-zero hi plane, so acc = +0 and the folded epilogue leaves fma(c_n, b_r, d_n) + bias_n whatever
    a_r is.  With the codes below every operation is EXACT in f32 (and in bf16 where the result is bf16), so `expect` is compared
    with ==.  b_r is a function of the row, c_n and d_n of the column; a_r is a second row code, never 0 or 1.

      plain   c_n, bias_n codes of 8 bits in (1, 4], d_n a code times 4: c b has 16 bits, the sums stay below 64 with a grain of
              2^-14: 20 bits of 24
      heads   the result must fit bf16's 8 bits: c-columns have d = 0 and c = +-2^e (result +-2^e b_r, times q_scale = 2^-3 in
              Q), d-columns have c = 0 and d = the column's code; the kind alternates inside a lane's four columns
      swiglu  silu(x1) == x1 exactly in f32 once x1 >= 32 (1 + e^-32 rounds to 1).  variant 0: x1 = 32 + 32 (d + bias), the codes
              in x2 as in `heads`;  variant 1: x2 = 0 + 0 + bias = 1 and the codes in x1, c = 2^5 or 2^6 and b_r > 0 in c-columns,
              32 |code| in d-columns -- both halves of the interleaved 16-row groups are probed
    -> the call, with `expect` in the epilogue's output shape and `coef_prev` (the row codes of another call)."""
    r, n = np.arange(M), np.arange(N)
    signed = epilogue != "swiglu"
    coef = np.stack([row_code(r, 1), row_code(r, 0, signed)], 1)
    coef_prev = np.stack([row_code(r, 3), row_code(r, 2, signed)], 1)
    colcode = _code((37 * n + 11) % 512)
    kind = _col_kind(n)
    bias = None
    if epilogue == "plain":
        c, d, bias = colcode, 4 * _code((53 * n + 7) % 512), _code((29 * n + 3) % 512)
    elif epilogue == "heads":
        c, d = np.where(kind, _pow2_col(n, -1, 4), 0.0), np.where(kind, 0.0, colcode)
    elif epilogue == "swiglu":
        is_x1 = (n // 16) % 2 == 0
        if variant == 0:
            c = np.where(is_x1, 0.0, np.where(kind, _pow2_col(n, -1, 4), 0.0))
            d = np.where(is_x1, 32.0, np.where(kind, 0.0, colcode))
            bias = np.where(is_x1, 32.0, 0.0)
        else:
            c = np.where(is_x1 & kind, np.abs(_pow2_col(n, 5, 2)), 0.0)
            d = np.where(is_x1 & ~kind, 32 * np.abs(colcode), 0.0)
            bias = np.where(is_x1, 0.0, 1.0)
    else:
        raise ValueError(epilogue)
    f32 = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float32)
    call = dict(h=np.zeros((M, K), np.float32), wg=_gauss_weights(N, K, 5), coef=f32(coef), coef_prev=f32(coef_prev), c=f32(c), d=f32(d),
                bias=f32(bias), heads=heads, tokens=tokens, q_scale=q_scale, family="index", epilogue=epilogue)
    call["expect"] = index_expect(call, epilogue)
    return call


def index_expect(call, epilogue):
    """what an all-zero hi plane must give, in float64 (every step is exact, asserted by tests/test_fold_probes_cpu.py)"""
    b = np.asarray(call["coef"], np.float64)[:, 1][:, None]
    pre = np.asarray(call["c"], np.float64)[None, :] * b + np.asarray(call["d"], np.float64)[None, :]
    if call.get("bias") is not None:
        pre = pre + np.asarray(call["bias"], np.float64)[None, :]
    if epilogue == "plain":
        out = pre
    elif epilogue == "heads":
        out = pre.copy()
        out[:, :call["heads"] * 64] *= call["q_scale"]
    else:
        i1, i2 = swiglu_cols(pre.shape[1] // 2)
        assert (pre[:, i1] >= 32).all()
        out = pre[:, i1] * pre[:, i2]
    out32 = out.astype(np.float32)
    assert np.array_equal(out32.astype(np.float64), out) and (epilogue == "plain" or is_bf16(out32))
    return out32


def _hash01(seed, r, salt):
    """splitmix64 of (seed, r, salt) -> uniform [0, 1): a function of the row index with no period"""
    with np.errstate(over="ignore"):
        z = (np.asarray(r, np.uint64) + np.uint64(seed) * np.uint64(0xD1B54A32D192ED03) + np.uint64(salt) * np.uint64(0x9E3779B97F4A7C15)
             + np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) / float(1 << 53)


def hetero_rows(M, K, seed=0):
    """-> (x [M, K] float32, mean [M], std [M]): row r is mean_r + std_r * normal with std log-uniform in [2^-3, 2^4] and the mean
    in +-[0, 8] std, both hashed from r"""
    r = np.arange(M)
    std = np.exp2(-3.0 + 7.0 * _hash01(seed, r, 1))
    mean = (16.0 * _hash01(seed, r, 2) - 8.0) * std
    z = np.random.default_rng([11, seed, K]).standard_normal((M, K), dtype=np.float32)
    return (mean[:, None] + std[:, None] * z).astype(np.float32), mean, std


def _gauss_weights(N, K, seed):
    return bf16_round(np.random.default_rng([13, seed, K]).standard_normal((N, K), dtype=np.float32) * np.float32(K ** -0.5))


def ln_coef64(h, eps=1e-5):
    """float64 (rstd, -rstd * mean) of the rows of h"""
    h = np.asarray(h, np.float64)
    rstd = 1.0 / np.sqrt(h.var(1) + eps)
    return np.stack([rstd, -rstd * h.mean(1)], 1)


def hetero_call(epilogue, M, N, K, seed=0, heads=8, tokens=256, q_scale=0.125):
    """The `hetero` family: realistic numerics with rows of very different statistics (hetero_rows), gamma per input column
    log-uniform in [0.25, 4], beta in +-2, weights K^-0.5-scaled normals, wg = bf16(gamma w), c = sum_k wg (of the rounded values,
    packing.ln_fold), d = sum_k beta w, a non-zero bias.  coef is the f32 rounding of the float64 statistics here; the GPU test
    replaces it with what pmhip_ln_coef computes.  coef_prev: the statistics of another row set of the same shape."""
    rng = np.random.default_rng([17, seed, N, K])
    h = bf16_round(hetero_rows(M, K, seed)[0])
    gamma = np.exp2(rng.uniform(-2.0, 2.0, K)).astype(np.float32)
    beta = rng.uniform(-2.0, 2.0, K).astype(np.float32)
    w = _gauss_weights(N, K, seed)
    wg = bf16_round(w * gamma[None, :])
    c = wg.astype(np.float64).sum(1).astype(np.float32)
    d = (w.astype(np.float64) * beta[None, :]).sum(1).astype(np.float32)
    bias = None if epilogue == "heads" else (0.5 + rng.standard_normal(N)).astype(np.float32)
    coef_prev = ln_coef64(bf16_round(hetero_rows(M, K, seed + 1000)[0])).astype(np.float32)
    return dict(h=h, wg=wg, coef=ln_coef64(h).astype(np.float32), coef_prev=coef_prev, c=c, d=d, bias=bias, heads=heads, tokens=tokens,
                q_scale=q_scale, family="hetero", epilogue=epilogue)


# ---------------------------------------------------------------------------------------------------------------- emulation

def fault_applies(fault, call, walk):
    M = call["h"].shape[0]
    if fault == "other_half_coef":
        return M % 256 == 0
    if fault == "previous_tile_coef":
        return bool((walk.previous_m() != np.arange(walk.tiles_m)[:, None]).any())
    if fault == "drop_bias":
        return call.get("bias") is not None
    return True


def faulted_rows(fault, call, walk):
    """boolean [M]: the rows whose coefficients a row fault replaces by those of ANOTHER row (in at least one column)"""
    M = call["h"].shape[0]
    r = np.arange(M)
    if fault == "next_row_coef":
        return r < M - 1
    if fault == "group_first_row_coef":
        return r % 16 != 0
    if fault in ("other_half_coef", "coef_from_previous_call"):
        return np.ones(M, bool)
    if fault == "previous_tile_coef":
        moved = (walk.previous_m() != np.arange(walk.tiles_m)[:, None]).any(1)
        return moved[r // walk.tile]
    raise ValueError(fault)


def _fma32(x, y, z):
    """float32 fma(x, y, z): the product of two float32 is exact in float64"""
    return (np.asarray(x, np.float64) * np.asarray(y, np.float64) + np.asarray(z, np.float64)).astype(np.float32)


def emulate(call, epilogue, fault=None, walk=None, round_out=True):
    """The folded epilogue in numpy float32 (ln_apply4: t = fma(c, b, d), o = fma(a, acc, t); then bias, scale, gate, rounding as
    gemm_common.h wave_epilogue does them), on a float32 matrix product.  -> the output in the epilogue's shape.

    fault: None or one of FAULTS --
      next_row_coef            row r uses the coefficients of row r + 1 (the last one its own)
      group_first_row_coef     every row of a 16-row MFMA group uses the group's first row
      other_half_coef          rows r and r ^ 128 exchange coefficients (the two wave rows `wm` of the 256x256 kernel)
      previous_tile_coef       a tile uses the coefficients that its workgroup's PREVIOUS tile left in the scratch (`walk`)
      coef_from_previous_call  the coefficients of a different row set of the same shape (call['coef_prev'])
      next_col_cd, col_plus_4_cd, col_plus_16_cd, col_plus_64_cd    the column uses c, d of the column 1, 4, 16, 64 further (mod N)
      swap_c_d                 c and d change places
      drop_bias                the bias is not added
    round_out = False: the bf16 epilogues return the float32 value in front of the output rounding."""
    assert fault is None or fault in FAULTS, fault
    h, wg = np.asarray(call["h"], np.float32), np.asarray(call["wg"], np.float32)
    M, N = h.shape[0], wg.shape[0]
    coef = np.asarray(call["coef_prev"] if fault == "coef_from_previous_call" else call["coef"], np.float32)
    c, d = np.asarray(call["c"], np.float32), np.asarray(call["d"], np.float32)
    bias = None if call.get("bias") is None or fault == "drop_bias" else np.asarray(call["bias"], np.float32)
    r, n = np.arange(M), np.arange(N)
    rows = r[:, None]
    if fault == "next_row_coef":
        rows = np.minimum(r + 1, M - 1)[:, None]
    elif fault == "group_first_row_coef":
        rows = (r & ~15)[:, None]
    elif fault == "other_half_coef":
        rows = (r ^ 128)[:, None]
    elif fault == "previous_tile_coef":
        pm = walk.previous_m()                                       # [tiles_m, tiles_n]
        rows = pm[r // walk.tile][:, n // walk.tile] * walk.tile + (r % walk.tile)[:, None]           # [M, N]
    if fault in _COL_SHIFT:
        c, d = c[(n + _COL_SHIFT[fault]) % N], d[(n + _COL_SHIFT[fault]) % N]
    elif fault == "swap_c_d":
        c, d = d, c
    a, b = coef[:, 0][rows], coef[:, 1][rows]                        # [M, 1] or [M, N]
    acc = h @ wg.T if h.any() else np.zeros((M, N), np.float32)
    o = _fma32(a, acc, _fma32(c[None, :], b, d[None, :]))
    if epilogue == "plain":
        return o if bias is None else o + bias[None, :]
    if epilogue == "heads":
        inner = call["heads"] * 64
        o[:, :inner] *= np.float32(call["q_scale"])
        return bf16_round(o) if round_out else o
    if epilogue == "swiglu":
        if bias is not None:
            o = o + bias[None, :]
        i1, i2 = swiglu_cols(N // 2)
        x1, x2 = o[:, i1], o[:, i2]
        with np.errstate(over="ignore"):                              # silu_mul_fast: x1 * rcp(1 + exp2(-x1 log2 e)) * x2
            g = x1 * (np.float32(1.0) / (np.float32(1.0) + np.exp2(x1 * np.float32(-LOG2E)))) * x2
        return bf16_round(g) if round_out else g
    raise ValueError(epilogue)


# ---------------------------------------------------------------------------------------------------------------- row statistics

def parts64(hi):
    """float64 partial statistics of a hi plane [M, D]: (sum, sum of squares about the part's own mean) of each 64-column part,
    [M, D / 64, 2] -- what pmhip_gemm_hilo_stats leaves for pmhip_ln_coef_parts"""
    M, D = hi.shape
    p = np.asarray(hi, np.float64).reshape(M, D // 64, 64)
    return np.stack([p.sum(-1), ((p - p.mean(-1, keepdims=True)) ** 2).sum(-1)], -1)


def stat_bounds(hi, eps=1e-5):
    """Element-wise bounds on the f32 row statistics of a hi plane [M, D], each relative to the row's (or part's) OWN scale, so
    that they mean the same for a row of spread 2^-3 and one of spread 2^4 with a mean of 8 spreads.  g = 65 EPS stands for a sum
    of 64 f32 terms in any order plus one more operation.

      part sum      |s - s64| <= g sum|h|                                        (64 terms, partial sums at most sum|h|)
      part square   the part mean m' = s / 64 carries dm <= g mean|h|.  Each term (h - m')^2 is a subtraction, and a fused
                    multiply-add into the running sum: the sum of the rounded terms is within g sum (h - m')^2, and
                    sum (h - m')^2 = sum (h - m)^2 + 64 dm^2 <= 2 sum (h - m)^2 + ..., so
                    |q - q64| <= 4 g sum (h - m)^2 + 64 (g mean|h|)^2
      rstd          m2 = sum_j (q_j + 64 (m_j - mean)^2) is a sum of D squares up to a relative error of 4 g for the parts and D / 64
                    + 8 operations of the tree, and rstd = (m2 / D + eps)^-1/2 halves a relative error: with the division, the
                    square root and the reciprocal   |rstd / rstd64 - 1| <= (D / 2 + 16) EPS
                    (the centred squares are sums of non-negative terms: no cancellation, so the bound is relative)
      b = -rstd mean   the mean is a sum of D terms: |dmean| <= (D + 16) EPS mean|h|; with rstd's relative error and the product:
                    |b - b64| <= |b64| (D / 2 + 16) EPS + rstd (D + 16) EPS mean|h| + EPS |b|
    -> dict(part_sum [M, D/64], part_sq [M, D/64], rstd_rel (a number), b [M]) and the float64 values (parts, coef)."""
    M, D = hi.shape
    h = np.asarray(hi, np.float64)
    p = h.reshape(M, D // 64, 64)
    g = 65 * EPS
    parts = parts64(hi)
    coef = ln_coef64(hi, eps)
    rstd_rel = (D / 2 + 16) * EPS
    mabs = np.abs(h).mean(1)
    b_abs = np.abs(coef[:, 1]) * rstd_rel + coef[:, 0] * (D + 16) * EPS * mabs + EPS * np.abs(coef[:, 1])
    return dict(part_sum=g * np.abs(p).sum(-1), part_sq=4 * g * parts[..., 1] + 64 * (g * np.abs(p).mean(-1)) ** 2, rstd_rel=rstd_rel, b=b_abs,
                parts=parts, coef=coef)


def parts_f32(hi):
    """gemm_common.h's row statistics in numpy float32: the 64 values of a part are summed 8 per lane and then across 8 lanes, the
    squares about sum / 64 are accumulated by fused multiply-adds in the same order"""
    M, D = hi.shape
    p = np.asarray(hi, np.float32).reshape(M, D // 64, 8, 8)
    lane = ((p[..., 0] + p[..., 1]) + (p[..., 2] + p[..., 3])) + ((p[..., 4] + p[..., 5]) + (p[..., 6] + p[..., 7]))
    tree = lambda v: ((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])) + ((v[..., 4] + v[..., 5]) + (v[..., 6] + v[..., 7]))
    sm = tree(lane)
    pm = sm * np.float32(1.0 / 64.0)
    q = np.zeros(lane.shape, np.float32)
    for j in range(8):
        a = p[..., j] - pm[..., None]
        q = _fma32(a, a, q)
    return np.stack([sm, tree(q)], -1)


def coef_from_parts_f32(parts, eps=1e-5):
    """common.h lnp_* / ln_coef_row in numpy float32: part j is paired with part j + 8 (missing parts count as zero), the eight
    pair values are summed as ((0+1)+(2+3)) + ((4+5)+(6+7))"""
    parts = np.asarray(parts, np.float32)
    M, nparts, _ = parts.shape
    assert 0 < nparts <= 16
    pad = np.zeros((M, 16, 2), np.float32)
    pad[:, :nparts] = parts
    live = (np.arange(16) < nparts)[None, :]
    tree = lambda v: ((v[:, 0] + v[:, 1]) + (v[:, 2] + v[:, 3])) + ((v[:, 4] + v[:, 5]) + (v[:, 6] + v[:, 7]))
    cnt = np.float32(nparts * 64)
    mean = tree(pad[:, :8, 0] + pad[:, 8:, 0]) / cnt
    dd = pad[..., 0] * np.float32(1.0 / 64.0) - mean[:, None]
    term = np.where(live, _fma32(np.float32(64.0) * dd, dd, pad[..., 1]), np.float32(0.0)).astype(np.float32)
    m2 = tree(term[:, :8] + term[:, 8:])
    rstd = np.float32(1.0) / np.sqrt(m2 / cnt + np.float32(eps))
    return np.stack([rstd, -rstd * mean], 1).astype(np.float32)
