"""Probes for the GEMMs WITHOUT a folded LayerNorm: the residual-stream producers (pmhip_gemm_hilo, _stats, _center), the f32
residual pmhip_gemm, and the unfolded plain, head-split and SwiGLU calls -- in the style of tests/fold_probes.py: a float64
reference built from exactly what the kernel is given, a family that is compared bit for bit, a family held element-wise to a
derived bound, and a numpy float32 restatement of the epilogues that can be made wrong on purpose.

No GPU and no torch in here: tests/test_gemm_probes_cpu.py proves on the CPU that every fault of FAULTS is rejected by the family
it names; tests/test_gpu_gemm_probes.py holds the kernels to the same two checks (check_selector, check_hetero).

A call is a dict.  a [M, K], w [N, K] float32 arrays of values the compute dtype holds exactly; bias [N] or None.  kind:
    'pair'    the hi/lo producer: res_hi, res_lo [M, N] bf16 planes (the kernel is given their first res_rows rows and reads row
              r % res_rows), center_coef [M, 2] or None with center_extra, shift0 [M] and shift_mode (0: no shift buffer), stats.
              x = (acc + bias) + ((res_hi + res_lo) - cen), cen = center_extra - coef_y * rcp(coef_x) (0 without centring);
              hi = bf16(x), lo = bf16(x - hi); shift <- 0 (mode 1) or shift0 + cen (mode 2), written by the wave of column block 0;
              parts [M, N / 64, 2] = (sum, centred sum of squares) of each 64-column part of the NEW hi plane
    'f32res'  out f32 = (acc + bias) + res[r % res_rows], res [M, N] float32
    'plain'   out f32 = acc + bias
    'heads'   N = 3 * heads * 64 columns q | k | v, q times q_scale, bf16, no bias (flat [M, N]: fold_probes.heads_to_flat)
    'swiglu'  N = 2 * Hp packed columns, silu(x1) * x2 in bf16, [M, Hp]
Results are dicts with the keys the kind has: out | hi, lo, shift, parts.
"""
import numpy as np

import fold_probes as F
from fold_probes import (EPS, U, Walk, _code, _gauss_weights, bf16_round, first_difference, heads_to_flat, hetero_rows,      # noqa: F401
                         is_bf16, row_code, stat_bounds, swiglu_cols, worst_ratio)

LOG2E = 1.4426950408889634
KINDS = ("pair", "f32res", "plain", "heads", "swiglu")

# kernel selection for ln == NULL, restated from dispatch() (csrc/gemm.hip), pm_gemm2b_supported (csrc/gemm2b.hip),
# pm_gemm256_supported and launch256() (csrc/gemm256.hip)
MIN_TILES_2B = 192            # at least this many 256x128 tiles for the two-workgroups-per-CU kernel
MIN_TILES_256 = 96            # at least this many 256x256 tiles for the 256x256 kernel
RES_KMIN_256 = 1024           # ... and with a residual, K at least this
PERSIST256 = 256              # more 256x256 tiles than this: 256 persistent workgroups walk them
DEEP128_MAX_TILES = 256       # deep128(): at most this many 128x128 tiles, and K >= 256 -> the four-stage, eight-wave form
CHUNK128, CHUNK256, CHUNK2B = 8, 6, 12
ROUTES = ("128x2", "128x4", "2b", "256", "256p", "f32")

# producers (the hi/lo pair, and the same shapes with an f32 residual): the smallest shapes per route, with the edges that route
# has -- ragged M and N and N % 64 == 0 for the statistics on the 128x128 kernels, 272 tiles and M no multiple of 256 for the
# two-stage form, K = 64 (one K-tile), 192 (three) and N = 384 (three tile columns) for the 2b kernel, 260 tiles (four
# workgroups walk two) for the persistent one
PRODUCER_SHAPES = {
    "128x2": [(300, 200, 128), (300, 192, 128), (2176, 2048, 256)],
    "128x4": [(300, 200, 256), (300, 192, 256)],
    "2b": [(6144, 1024, 64), (6144, 1024, 192), (16384, 384, 64)],
    "256": [(6144, 1024, 1024)],
    "256p": [(16640, 1024, 1024)],
}
F32_SHAPE = (300, 200, 128)
# unfolded plain / heads / swiglu: fold_probes.SHAPES, which land on these routes without a fold
UNFOLDED_ROUTE = {"A": "128x4", "B": "128x2", "C": "256", "D": "256p"}
# head split with 200 tokens per image (tokens_pad 256) on the two FULL routes: the wave's rows cross an image (!nowrap Q / K arm)
# and the 64-token V^T blocks are not `whole`
HEADS_T200 = {"256": (6400, 1536, 128), "256p": (12800, 1536, 128)}
HEADS, TOKENS, Q_SCALE = F.HEADS, F.TOKENS, F.Q_SCALE


# ---------------------------------------------------------------------------------------------------------------- geometry

def _supported2b(M, N, K):
    return M % 256 == 0 and N % 128 == 0 and K % 64 == 0 and (M // 256) * (N // 128) >= MIN_TILES_2B


def _supported256(M, N, K, residual):
    if M % 256 or N % 256 or K % 64 or K < 128 or M * K * 2 >= 2 ** 31 or N * K * 2 >= 2 ** 31:
        return False
    return (M // 256) * (N // 256) >= MIN_TILES_256 and (not residual or K >= RES_KMIN_256)


def route_of(M, N, K, residual, dtype="bf16"):
    """dispatch() for ln == NULL.  residual: an EPI_STD call with a residual (f32, or the hi/lo pair)"""
    if dtype == "f32":
        return "f32"
    s256 = _supported256(M, N, K, residual)
    if residual and not s256 and _supported2b(M, N, K):
        return "2b"
    if s256:
        return "256p" if (M // 256) * (N // 256) > PERSIST256 else "256"
    return "128x4" if -(-M // 128) * -(-N // 128) <= DEEP128_MAX_TILES and K >= 256 else "128x2"


class Walk2b:
    """the walk of gemm2b.hip: 256x128 tiles, one workgroup per tile (the interface of fold_probes.Walk)"""

    def __init__(self, M, N):
        self.M, self.N, self.tile_m, self.tile_n, self.route = M, N, 256, 128, "2b"
        self.tiles_m, self.tiles_n = M // 256, N // 128
        nt = self.tiles_m * self.tiles_n
        self.grid = nt
        idx = np.arange(nt)
        tm, tn = F._tile_of_block(F._xcd_remap(idx, nt), self.tiles_m, self.tiles_n, CHUNK2B)
        self.order = np.full((self.tiles_m, self.tiles_n), -1, np.int64)
        self.order[tm, tn] = idx
        assert (self.order >= 0).all(), "the tile walk is not a bijection"
        self.tm, self.tn = tm, tn

    def step(self):
        return self.order // self.grid

    def describe(self, r, n):
        tm, tn = r // 256, n // 128
        return f"route 2b, 256x128 tile (m, n) = ({tm}, {tn}), launch index {int(self.order[tm, tn])} (one tile per workgroup)"


def walk_of(M, N, K, residual, dtype="bf16", grid=PERSIST256):
    r = route_of(M, N, K, residual, dtype)
    if r == "2b":
        return Walk2b(M, N)
    if r in ("256", "256p"):
        return Walk(M, N, 256, CHUNK256, grid, r)
    return Walk(M, N, 128, CHUNK128, None, r)


def tile_shape(walk):
    return (walk.tile_m, walk.tile_n) if hasattr(walk, "tile_m") else (walk.tile, walk.tile)


def previous_tile(walk):
    """([tiles_m, tiles_n] tile row, tile column) of the tile the same workgroup ran before (its own where it is the first):
    fold_probes.Walk.previous_m and its n analogue"""
    prev = np.where(walk.order >= walk.grid, walk.order - walk.grid, walk.order)
    return walk.tm[prev], walk.tn[prev]


def walked_blocks(walk):
    """the 256-row blocks a restricted float64 reference of a persistent shape must hold: every block with a tile whose walk step
    is >= 1, plus the first and the last -> sorted row indices"""
    tiles = set(np.nonzero((walk.step() >= 1).any(1))[0].tolist()) | {0, walk.tiles_m - 1}
    return np.concatenate([np.arange(t * walk.tile, (t + 1) * walk.tile) for t in sorted(tiles)])


# ---------------------------------------------------------------------------------------------------------------- faults

# fault -> (the kinds it exists in, the families that must reject it).  tests/test_gemm_probes_cpu.py asserts both.
_ALL, _RES, _PAIR = KINDS, ("pair", "f32res"), ("pair",)
FAULTS = {
    # K loop.  first / last K-tile: the peeled tiles of gemm256.hip; foreign: K-tile 0 of the tile the persistent workgroup ran before
    "drop_first_ktile": (_ALL, ("selector",)), "drop_last_ktile": (_ALL, ("selector",)), "double_last_ktile": (_ALL, ("selector",)),
    "foreign_ktile0": (_ALL, ("selector",)),
    # residual: row r + 1; rows r and r ^ 128 exchanged; row r + 16 (the ring slot of the next slice); r instead of r % res_rows;
    # the lo plane of the other column of the packed word
    "res_next_row": (_RES, ("selector", "hetero")), "res_other_half": (_RES, ("selector", "hetero")),
    "res_next_slice": (_RES, ("selector", "hetero")), "res_no_modulo": (_RES, ("selector", "hetero")),
    "res_lo_other_col": (_PAIR, ("selector", "hetero")),
    # bias: of the column 1, 4, 8, 64 further (mod N); not added
    "bias_col_1": (_ALL, ("selector", "hetero")), "bias_col_4": (_ALL, ("selector", "hetero")), "bias_col_8": (_ALL, ("selector", "hetero")),
    "bias_col_64": (_ALL, ("selector", "hetero")), "drop_bias": (_ALL, ("selector", "hetero")),
    # centre: coefficient of row r + 1, of the 16-row group's first row; center_extra dropped; shift mode 2 behaving as mode 1;
    # the shift written by a wave of a column block other than 0 (which never loaded the running value: shift <- cen).  The value
    # check of `hetero` uses the shift that comes back as the centre, so only its shift bound sees the first three; the last one
    # is invisible to it (shift0 = 0 there)
    "center_next_row": (_PAIR, ("selector", "hetero")), "center_group_first_row": (_PAIR, ("selector", "hetero")),
    "drop_center_extra": (_PAIR, ("selector", "hetero")), "shift_mode2_as_1": (_PAIR, ("selector", "hetero")),
    "shift_from_other_block": (_PAIR, ("selector",)),
    # statistics: written to part + 1 (mod N / 64); taken from the rows of the previous 16-row slice
    "stats_next_part": (_PAIR, ("selector", "hetero")), "stats_previous_slice": (_PAIR, ("selector", "hetero")),
    # output: the hi plane truncated instead of rounded to nearest even (hi + lo still reproduces x)
    "truncate_hi": (_PAIR, ("selector", "hetero")),
}
_K_FAULTS = ("drop_first_ktile", "drop_last_ktile", "double_last_ktile", "foreign_ktile0")
_BIAS_SHIFT = {"bias_col_1": 1, "bias_col_4": 4, "bias_col_8": 8, "bias_col_64": 64}


def fault_applies(fault, call, kind, walk):
    if kind not in FAULTS[fault][0]:
        return False
    M = call["a"].shape[0]
    if fault == "foreign_ktile0":
        pm, pn = previous_tile(walk)
        return bool(((pm != np.arange(walk.tiles_m)[:, None]) | (pn != np.arange(walk.tiles_n)[None, :])).any())
    if fault == "res_other_half":                                   # (a row modulo that divides the distance hides the fault)
        return M % 256 == 0 and 128 % call["res_rows"] != 0
    if fault == "res_next_slice":
        return 16 % call["res_rows"] != 0
    if fault == "res_no_modulo":
        return 0 < call["res_rows"] < M
    if fault.startswith("bias") or fault == "drop_bias":
        return call.get("bias") is not None
    if fault in ("center_next_row", "center_group_first_row", "drop_center_extra"):
        return call.get("center_coef") is not None
    if fault in ("shift_mode2_as_1", "shift_from_other_block"):
        return call.get("shift_mode") == 2
    if fault.startswith("stats"):
        return bool(call.get("stats"))
    return True


# ---------------------------------------------------------------------------------------------------------------- the two families

def _split(x):
    hi = bf16_round(x)
    return hi, bf16_round(np.asarray(x, np.float32) - hi)


def _kstep(dtype):
    return 64 if dtype == "bf16" else 32          # elements of k per 128-byte tile row


def selector_k(r, K, kstep):
    """(k1, k2) of row r: the two columns of A that hold a one -- k1 in the first half of the first K-tile, k2 in the second half
    of the last one (for K = kstep: the two halves of the only K-tile); both change with the row, its 16-row group and its
    256-row block"""
    r, half = np.asarray(r, np.int64), kstep // 2
    return (7 * r + 3 * (r >> 4) + 5 * (r >> 8)) % half, K - half + (11 * r + 5 * (r >> 4) + 3 * (r >> 8) + 1) % half


def selector_call(kind, M, N, K, dtype="bf16", res_rows=0, center=0, stats=False, heads=HEADS, tokens=TOKENS, q_scale=Q_SCALE):
    """The `selector` family.  A has exactly two ones per row (selector_k), W[n, k] is a _code of (n, k, k // 64): 8 significant
    bits, magnitude in (1, 4] -- so acc[r, n] = W[n, k1] + W[n, k2] EXACTLY, and a dropped, doubled or foreign K-tile changes an
    identifiable element.  bias: a column code; residual: multiples of 2^-10 of magnitude below 64 (16 significant bits: hi + lo
    exactly); centring (center = shift mode 1 or 2): a_r = 1, b_r = 8 * row_code, center_extra = 0.25, shift0 a row code.  Every
    f32 operation of the epilogue is then exact (magnitudes below 109 on a grain of 2^-10: 17 bits; the 64-term sums of the new hi
    plane stay below 2^13 on that grain: 23 bits, in any order) -- asserted by expect_selector.
    heads: the f32 value acc * q_scale is exact, the stored bf16 its rounding.  swiglu: the bias of the x1 columns is 48, so
    x1 >= 40 and silu(x1) == x1 in f32 (1 + e^-40 rounds to 1, its reciprocal is 1); the bias of the x2 columns is the column
    code, and x1 * x2 has at most 24 bits."""
    assert kind in KINDS and (kind in ("pair", "f32res") or not (res_rows or center or stats))
    r, n, ks = np.arange(M), np.arange(N), _kstep(dtype)
    k1, k2 = selector_k(r, K, ks)
    a = np.zeros((M, K), np.float32)
    a[r, k1] = 1.0
    a[r, k2] = 1.0
    kk = np.arange(K)
    w = _code((37 * n[:, None] + 101 * kk[None, :] + 59 * (kk[None, :] // 64)) % 512)
    colcode = _code((37 * n + 11) % 512)
    call = dict(a=a, w=w, bias=colcode, k1=k1, k2=k2, kstep=ks, dtype=dtype, family="selector", kind=kind, res_rows=0, heads=heads,
                tokens=tokens, q_scale=q_scale)
    if kind == "heads":
        call["bias"] = None
    elif kind == "swiglu":
        call["bias"] = np.where((n // 16) % 2 == 0, np.float32(48.0), colcode).astype(np.float32)
    if kind in ("pair", "f32res"):
        q = (r[:, None] * 40503 + n[None, :] * 30011 + (r[:, None] >> 4) * 977 + (n[None, :] >> 3) * 131) % 131071 - 65535
        res = (q * 2.0 ** -10).astype(np.float32)
        call["res_rows"] = res_rows or M
        if kind == "f32res":
            call["res"] = res
        else:
            call["res_hi"], call["res_lo"] = _split(res)
            assert np.array_equal(call["res_hi"].astype(np.float64) + call["res_lo"], res)
            call.update(stats=stats, shift_mode=center, center_coef=None, center_extra=0.0, shift0=None)
            if center:
                assert not res_rows
                call.update(center_coef=np.stack([np.ones(M, np.float32), 8 * row_code(r)], 1).astype(np.float32), center_extra=0.25,
                            shift0=row_code(r, 1).astype(np.float32))
    return call


def hetero_call(kind, M, N, K, center=False, stats=True, res_rows=0, seed=0):
    """The `hetero` family (producers): the residual stream is hetero_rows(M, N) -- row spreads 2^-3 .. 2^4, means out to 8
    spreads; the rows of A are scaled by the row's spread, the weights are K^-0.5-scaled normals, the bias 0.5 * normal.  With
    centring: center_coef = the f32 LayerNorm pair of the residual hi plane, center_extra = the mean of the bias, shift0 = 0 and
    shift mode 2, so that the centre the kernel used comes back in `shift`."""
    assert kind in ("pair", "f32res")
    x, _, std = hetero_rows(M, N, seed)
    rng = np.random.default_rng([23, seed, M, N, K])
    a = bf16_round((std[:, None] * rng.standard_normal((M, K))).astype(np.float32))
    bias = (0.5 * rng.standard_normal(N)).astype(np.float32)
    call = dict(a=a, w=_gauss_weights(N, K, seed), bias=bias, kstep=64, dtype="bf16", family="hetero", kind=kind, res_rows=res_rows or M)
    if kind == "f32res":
        call["res"] = x
        return call
    call["res_hi"], call["res_lo"] = _split(x)
    call.update(stats=stats, shift_mode=0, center_coef=None, center_extra=0.0, shift0=None)
    if center:
        assert not res_rows
        h = call["res_hi"].astype(np.float64)
        rstd = 1.0 / np.sqrt(h.var(1) + 1e-5)
        call.update(center_coef=np.stack([rstd, -rstd * h.mean(1)], 1).astype(np.float32), center_extra=float(np.float32(bias.mean())),
                    shift0=np.zeros(M, np.float32), shift_mode=2)
    return call


# ---------------------------------------------------------------------------------------------------------------- emulation

def _fma32(x, y, z):
    return (np.asarray(x, np.float64) * np.asarray(y, np.float64) + np.asarray(z, np.float64)).astype(np.float32)


def _acc32(call, fault, walk):
    a, w, ks = np.asarray(call["a"], np.float32), np.asarray(call["w"], np.float32), call["kstep"]
    K = a.shape[1]
    acc = a @ w.T
    if fault not in _K_FAULTS:
        return acc
    first, last = a[:, :ks] @ w[:, :ks].T, a[:, K - ks:] @ w[:, K - ks:].T
    if fault == "drop_first_ktile":
        return acc - first
    if fault == "drop_last_ktile":
        return acc - last
    if fault == "double_last_ktile":
        return acc + last
    pm, pn = previous_tile(walk)
    tm, tn = tile_shape(walk)
    for i in range(walk.tiles_m):
        for j in range(walk.tiles_n):
            if (pm[i, j], pn[i, j]) != (i, j):
                rs, cs = slice(i * tm, (i + 1) * tm), slice(j * tn, (j + 1) * tn)
                foreign = a[pm[i, j] * tm:(pm[i, j] + 1) * tm, :ks] @ w[pn[i, j] * tn:(pn[i, j] + 1) * tn, :ks].T
                acc[rs, cs] = acc[rs, cs] - first[rs, cs] + foreign
    return acc


def emulate(call, kind, fault=None, walk=None):
    """The HILO, f32-residual and unfolded epilogues of gemm_common.h wave_epilogue in numpy float32, on a float32 matrix product;
    fault: None or a key of FAULTS (walk: needed by foreign_ktile0).  -> the result dict of the kind."""
    assert fault is None or (fault in FAULTS and kind in FAULTS[fault][0]), (fault, kind)
    acc = _acc32(call, fault, walk)
    M, N = acc.shape
    r, n = np.arange(M), np.arange(N)
    bias = None if call.get("bias") is None or fault == "drop_bias" else np.asarray(call["bias"], np.float32)
    if fault in _BIAS_SHIFT:
        bias = bias[(n + _BIAS_SHIFT[fault]) % N]
    if kind == "heads":
        o = acc.copy()
        o[:, :call["heads"] * 64] *= np.float32(call["q_scale"])
        return dict(out=bf16_round(o))
    v = acc if bias is None else acc + bias[None, :]
    if kind == "plain":
        return dict(out=v)
    if kind == "swiglu":
        i1, i2 = swiglu_cols(N // 2)
        x1, x2 = v[:, i1], v[:, i2]
        with np.errstate(over="ignore"):                              # silu_mul_fast: x1 * rcp(1 + exp2(-x1 log2 e)) * x2
            return dict(out=bf16_round(x1 * (np.float32(1.0) / (np.float32(1.0) + np.exp2(x1 * np.float32(-LOG2E)))) * x2))
    R = call["res_rows"]
    rr = {"res_next_row": np.minimum(r + 1, M - 1), "res_other_half": r ^ 128, "res_next_slice": np.minimum(r + 16, M - 1)}.get(fault, r)
    rr = rr if fault == "res_no_modulo" else rr % R
    if kind == "f32res":
        return dict(out=v + np.asarray(call["res"], np.float32)[rr])
    rh, rl = np.asarray(call["res_hi"], np.float32)[rr], np.asarray(call["res_lo"], np.float32)[rr]
    if fault == "res_lo_other_col":
        rl = rl[:, n ^ 1]
    cen = np.zeros(M, np.float32)
    if call.get("center_coef") is not None:
        cr = {"center_next_row": np.minimum(r + 1, M - 1), "center_group_first_row": r & ~15}.get(fault, r)
        cc = np.asarray(call["center_coef"], np.float32)[cr]
        extra = np.float32(0.0 if fault == "drop_center_extra" else call["center_extra"])
        cen = _fma32(-cc[:, 1], np.float32(1.0) / cc[:, 0], extra)
    x = v + ((rh + rl) - cen[:, None])
    hi = bf16_round(x) if fault != "truncate_hi" else (np.ascontiguousarray(x).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    out = dict(hi=hi, lo=bf16_round(x - hi))
    mode = call.get("shift_mode", 0)
    if mode == 1 or (mode == 2 and fault == "shift_mode2_as_1"):
        out["shift"] = np.zeros(M, np.float32)
    elif mode == 2:
        out["shift"] = (np.float32(0.0) if fault == "shift_from_other_block" else np.asarray(call["shift0"], np.float32)) + cen
    if call.get("stats"):
        p = F.parts_f32(hi)
        if fault == "stats_next_part":
            p = np.roll(p, 1, axis=1)
        elif fault == "stats_previous_slice":
            p = p[np.maximum(r - 16, 0)]
        out["parts"] = p
    return out


# ---------------------------------------------------------------------------------------------------------------- selector: expectation and check

def _exact32(x, what):
    x32 = np.asarray(x, np.float64).astype(np.float32)
    assert np.array_equal(x32.astype(np.float64), x), f"selector family: {what} is not exact in float32"
    return x32


def expect_selector(call, kind, rows=None):
    """What the selector call must give, computed in float64 with every intermediate of the epilogue asserted to be a float32
    value (so every f32 operation of the kernel is exact and its order does not matter); `rows`: only these rows.
    -> the result dict (parts: only the part sums, [rows, N / 64]; the squares are held to stat_bounds)."""
    w = np.asarray(call["w"], np.float64)
    M, N = call["a"].shape[0], w.shape[0]
    r = np.arange(M) if rows is None else np.asarray(rows)
    acc = _exact32(w[:, call["k1"][r]].T + w[:, call["k2"][r]].T, "acc")
    if kind == "heads":
        o = acc.astype(np.float64)
        o[:, :call["heads"] * 64] *= call["q_scale"]
        return dict(out=bf16_round(_exact32(o, "acc * q_scale")))
    v = _exact32(acc + np.asarray(call["bias"], np.float64)[None, :], "acc + bias").astype(np.float64)
    if kind == "plain":
        return dict(out=v.astype(np.float32))
    if kind == "swiglu":
        i1, i2 = swiglu_cols(N // 2)
        assert (v[:, i1] >= 40).all()
        return dict(out=bf16_round(_exact32(v[:, i1] * v[:, i2], "x1 * x2")))
    rr = r % call["res_rows"]
    if kind == "f32res":
        return dict(out=_exact32(v + np.asarray(call["res"], np.float64)[rr], "v + residual"))
    res = _exact32(np.asarray(call["res_hi"], np.float64)[rr] + np.asarray(call["res_lo"], np.float64)[rr], "hi + lo").astype(np.float64)
    cen = np.zeros(len(r))
    if call["center_coef"] is not None:
        cc = np.asarray(call["center_coef"], np.float64)[r]
        assert (cc[:, 0] == 1.0).all()                                  # the reciprocal of 1.0 is taken to be 1.0
        cen = _exact32(call["center_extra"] - cc[:, 1], "centre").astype(np.float64)
    x = _exact32(v + _exact32(res - cen[:, None], "residual - centre"), "x").astype(np.float64)
    assert np.abs(x).max() < 109
    hi = bf16_round(x.astype(np.float32))
    lo = _exact32(x - hi, "x - hi")
    assert is_bf16(lo)
    out = dict(hi=hi, lo=lo)
    if call["shift_mode"] == 1:
        out["shift"] = np.zeros(len(r), np.float32)
    elif call["shift_mode"] == 2:
        out["shift"] = _exact32(np.asarray(call["shift0"], np.float64)[r] + cen, "shift0 + centre")
    if call["stats"]:
        g = hi.astype(np.float64).reshape(len(r), N // 64, 64) * 1024.0
        assert np.array_equal(g, np.round(g)) and np.abs(g).sum(-1).max() < 2 ** 24       # integers on the 2^-10 grain: exact in any order
        out["parts"] = _exact32(g.sum(-1) / 1024.0, "part sums")
    return out


def expect_selector_chunked(call, kind, chunk=2048):
    """expect_selector over all rows, `chunk` rows at a time (the float64 intermediates of a 16640 x 1024 call are 136 MB each)"""
    M = call["a"].shape[0]
    parts = [expect_selector(call, kind, np.arange(r0, min(r0 + chunk, M))) for r0 in range(0, M, chunk)]
    return {k: np.concatenate([p[k] for p in parts], 0) for k in parts[0]}


def _first_row_difference(got, want, what, walk):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    if not len(bad):
        return None
    r = int(bad[0])
    return (f"{what}: {len(bad)} rows differ (all of them: {len(bad) == len(want)}); first row {r}: got {float(got[r])!r} want {float(want[r])!r}; "
            f"{walk.describe(r, 0)}")


def check_selector(got, want, call, kind, walk, what=""):
    """-> the list of messages (empty: everything equals bit for bit, and the part squares are within stat_bounds), each naming
    the first wrong element, its tile and the tile's place in the workgroup's walk"""
    epi = "swiglu" if kind == "swiglu" else "plain"
    msgs = []
    for key in ("out", "hi", "lo"):
        if key in want:
            msgs.append(first_difference(got[key], want[key], epi, walk, f"{what} {key}"))
    if "shift" in want:
        msgs.append(_first_row_difference(got["shift"], want["shift"], f"{what} shift", walk))
    if "parts" in want:
        p = np.asarray(got["parts"])
        bad = p[..., 0] != want["parts"]
        if bad.any():
            r, j = (int(x) for x in np.argwhere(bad)[0])
            msgs.append(f"{what} part sums: {int(bad.sum())} differ; first (row, part) = ({r}, {j}): got {float(p[r, j, 0])!r} want "
                        f"{float(want['parts'][r, j])!r}; {walk.describe(r, j * 64)}")
        sb = stat_bounds(want["hi"])
        ratio, (r, j) = worst_ratio(p[..., 1], sb["parts"][..., 1], sb["part_sq"])
        if ratio > 1.0:
            msgs.append(f"{what} part squares: err / bound = {ratio:.3g} at (row, part) = ({r}, {j}): got {float(p[r, j, 1])!r} want "
                        f"{sb['parts'][r, j, 1]!r}; {walk.describe(r, j * 64)}")
    return [m for m in msgs if m]


# ---------------------------------------------------------------------------------------------------------------- hetero: reference and check

def reference(call, kind, cen=None, rows=None):
    """float64 reference x64 and the element-wise bound B of the f32 value, for `rows` (all by default).

    x64 = acc + bias + (r - cen), S[r, n] = sum_k |a_rk| |w_nk|; per f32 operation EPS = 2^-23, per bf16 rounding U = 2^-8.
      B = (K + 8) EPS S  +  4 EPS (|acc| + |bias| + |r| + |cen|)
          first term: the K-term accumulation (every partial sum is at most S); second: the bias add, the subtraction of the
          centre and the residual add, three roundings of values that are at most the sum of the four magnitudes, one EPS to
          spare (hi + lo of the residual pair is exact in f32).
    cen [M]: the centre the kernel used (its own `shift`, read back), or None."""
    M = call["a"].shape[0]
    r = np.arange(M) if rows is None else np.asarray(rows)
    a, w = np.asarray(call["a"], np.float64)[r], np.asarray(call["w"], np.float64)
    acc, S = a @ w.T, np.abs(a) @ np.abs(w).T
    bias = np.asarray(call["bias"], np.float64)[None, :]
    rr = r % call["res_rows"]
    res = np.asarray(call["res"], np.float64)[rr] if kind == "f32res" else np.asarray(call["res_hi"], np.float64)[rr] + np.asarray(call["res_lo"], np.float64)[rr]
    c = np.zeros((len(r), 1)) if cen is None else np.asarray(cen, np.float64)[r][:, None]
    K = a.shape[1]
    return acc + bias + (res - c), (K + 8) * EPS * S + 4 * EPS * (np.abs(acc) + np.abs(bias) + np.abs(res) + np.abs(c))


def shift_reference(call):
    """float64 centre from the f32 center_coef and its bound: cen = extra - y * rcp(x) is a hardware reciprocal (one ulp), a
    multiplication and a subtraction (or one fused multiply-add), values at most |extra| + |y / x|; one EPS to spare:
    |cen - cen64| <= 4 EPS (|extra| + |y / x|)"""
    cc = np.asarray(call["center_coef"], np.float64)
    m = cc[:, 1] / cc[:, 0]
    return call["center_extra"] - m, 4 * EPS * (abs(call["center_extra"]) + np.abs(m))


def check_hetero(got, call, kind, walk, rows=None, what=""):
    """The element-wise checks of the hetero family on a result dict -> (dict of largest err / bound per check, list of messages).
        f32      |out - x64| <= B
        pair     |hi + lo - x64| <= B + U^2 (|x64| + B)   and   |lo| <= U |hi|
        shift    (centred, mode 2, shift0 = 0)  |shift - cen64| <= its bound; the value check uses the shift as the centre
        parts    stat_bounds on the new hi plane
    rows: restrict the value check to these rows (the statistics, the shift and |lo| <= U |hi| always cover every row)."""
    M = call["a"].shape[0]
    r = np.arange(M) if rows is None else np.asarray(rows)
    ratios, msgs = {}, []

    def hold(name, ratio, where, detail):
        ratios[name] = round(ratio, 3)
        if not ratio <= 1.0:
            msgs.append(f"{what} {name}: err / bound = {ratio:.3g} at {where}; {detail}")

    cen = None
    if kind == "pair" and call.get("center_coef") is not None:
        cen = np.asarray(got["shift"], np.float64)
        c64, cb = shift_reference(call)
        ratio, (i, _) = worst_ratio(cen[:, None], c64[:, None], cb[:, None])
        hold("shift", ratio, f"row {i}", f"got {cen[i]!r} want {c64[i]!r}; {walk.describe(i, 0)}")
    x64, B = reference(call, kind, cen, r)
    if kind == "f32res":
        ratio, (i, j) = worst_ratio(np.asarray(got["out"])[r], x64, B)
        hold("out", ratio, f"(row, column) = ({int(r[i])}, {j})", f"got {float(got['out'][r[i], j])!r} want {x64[i, j]!r} bound {B[i, j]!r}; {walk.describe(int(r[i]), j)}")
        return ratios, msgs
    hi, lo = np.asarray(got["hi"], np.float64), np.asarray(got["lo"], np.float64)
    ratio, (i, j) = worst_ratio(hi[r] + lo[r], x64, B + U * U * (np.abs(x64) + B))
    hold("hi + lo", ratio, f"(row, column) = ({int(r[i])}, {j})", f"got {hi[r[i], j] + lo[r[i], j]!r} want {x64[i, j]!r}; {walk.describe(int(r[i]), j)}")
    ratio, (i, j) = worst_ratio(np.abs(lo), np.zeros_like(lo), U * np.abs(hi))
    hold("|lo| / U |hi|", ratio, f"(row, column) = ({i}, {j})", f"hi {hi[i, j]!r} lo {lo[i, j]!r}; {walk.describe(i, j)}")
    if call.get("stats"):
        sb = stat_bounds(got["hi"])
        p = np.asarray(got["parts"], np.float64)
        for k, name, bound in ((0, "part sum", sb["part_sum"]), (1, "part square", sb["part_sq"])):
            ratio, (i, j) = worst_ratio(p[..., k], sb["parts"][..., k], bound)
            hold(name, ratio, f"(row, part) = ({i}, {j})", f"got {p[i, j, k]!r} want {sb['parts'][i, j, k]!r}; {walk.describe(i, j * 64)}")
    return ratios, msgs
