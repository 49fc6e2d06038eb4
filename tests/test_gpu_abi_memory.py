"""The C ABI's memory contract (include/pmhip.h), operator by operator: leading dimensions wider than the payload, in place where
the header allows it, and outputs of exactly their extent.

Every case calls an entry point twice on the same values -- once contiguous, as the rest of the suite does (paintmind_amd.ops only
passes contiguous tensors and the engine always passes ld == width), once with every input in a NaN-framed buffer and every output
in a sentinel-framed buffer with ld > width (tests/abi_frames.py).  It is the same kernel, the same tile map and the same
arithmetic order, and nothing in the dispatch depends on a leading dimension while M * lda * 2 and N * ldw * 2 stay below 2^31, so
the two payloads must be BIT-IDENTICAL, and every element of every output frame outside its payload must be untouched.  Once per
route the contiguous result is also held against float64 with the tolerance tests/test_gpu_ops.py uses for that operator.

GEMM shapes walk every rung of gemm.hip's dispatch<EPI>() once; they are read off its predicates (deep128, fold_small,
pm_gemm256_supported, pm_gemm2b_supported) and the route is part of the test id:

    f32-128x128             f32 operands: 128x128 tiles, two LDS stages                                   300 x 200 x 128
    bf16-128x128-2stage     not whole 256-tiles, K < 256: two stages, four waves                          300 x 200 x 128
    bf16-128x128-4stage     at most 256 tiles of 128x128 and K >= 256: four stages, EIGHT waves           300 x 200 x 256
    bf16-256x256-2k         >= 96 tiles of 256x256; two K-tiles (the first and the last, both peeled)     6144 x 1024 x 128
    bf16-256x256-3k         the same, odd K-tile count                                                    6144 x 1024 x 192
    bf16-256x256-streamed   more tiles than the persistent grid (256 workgroups, at least the CU count):
                            a workgroup streams in a second tile                                           256 * (max(CUs, 256) / 4 + 1) x 1024 x 128
    bf16-256x256-residual   a residual GEMM takes the 256x256 kernel from K = 1024 (res_kmin)             6144 x 1024 x 1024
    bf16-256x256-residual-streamed   the same with the streamed row count: the second tile of a workgroup
                            reads and writes its residual in place too                                     (streamed rows) x 1024 x 1024
    bf16-2b                 256x128 tiles, two workgroups per CU: residual, >= 192 tiles, not served by
                            the 256x256 kernel (K < 1024 here)                                             12288 x 512 x 64
    bf16-2b-n384            the same kernel, N a multiple of 128 but not of 256.  192 tiles of 256x128
                            need M = 16384 at N = 384 (12288 x 384 would be 144 tiles: the 128x128 kernel) 16384 x 384 x 512
    fold-128x128-2stage     folded LayerNorm, at most 128 tiles of 256x256, K < 256; coef given           256 x 256 x 128
    fold-128x128-4stage     the same with K >= 256; with `parts` coef is written by the GEMM's prologue   256 x 256 x 256
    fold-256x256            folded, more than 128 tiles of 256x256                                         8448 x 1024 x 128
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import abi_frames as F
from abi_frames import bits, call, framed
from gpu_common import bf16_round, dev, n, rel_err, t
from oracle import paintmind_oracle as O
from paintmind_amd import _lib, ops
from paintmind_amd._lib import BF16, F32, PART_K, PART_Q, PART_V
from util import maxabs

pytestmark = pytest.mark.gpu

f32, bf16, i64 = torch.float32, torch.bfloat16, torch.int64
TDT = {F32: f32, BF16: bf16}


# ---------------------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------------------
class Layout:
    """One way of laying a call's operands out: contiguous (ld == width) or strided (ld = default_ld(width) unless given).  Either
    way every operand sits in a frame: inputs in NaN, outputs in the sentinel.  Arrays the ABI has no leading dimension for are
    `flat` in both layouts (guard rows only)."""

    def __init__(self, strided):
        self.strided, self.outs = strided, []

    def _ld(self, cols, ld):
        return cols if not self.strided else (F.default_ld(cols) if ld is None else ld)

    def inp(self, x, ld=None):
        return framed(x.shape[0], x.shape[1], ld=self._ld(x.shape[1], ld), dtype=x.dtype, payload=x,
                      fill="nan" if x.dtype.is_floating_point else "sentinel")

    def flat(self, x):
        x2 = x.reshape(1, -1) if x.dim() == 1 else x.reshape(-1, x.shape[-1])
        return framed(x2.shape[0], x2.shape[1], ld=x2.shape[1], dtype=x.dtype, payload=x2,
                      fill="nan" if x.dtype.is_floating_point else "sentinel")

    def out(self, rows, cols, dtype, payload=None, ld=None, flat=False):
        f = framed(rows, cols, ld=cols if flat else self._ld(cols, ld), dtype=dtype, payload=payload, fill="sentinel", device=dev())
        self.outs.append(f)
        return f

    def check(self):
        for i, f in enumerate(self.outs):
            f.assert_frame_untouched(f"{'strided' if self.strided else 'contiguous'} call, output {i}")


def same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = bits(a) != bits(b)
    if bool(bad.any()):
        idx = torch.nonzero(bad)[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {a.numel()} elements differ, the first at {idx}: "
                             f"{a[tuple(idx)].item()!r} != {b[tuple(idx)].item()!r}")


def both(run):
    """run(layout) -> list of result tensors.  Contiguous, then strided: frames untouched, results bit-identical.  -> the results"""
    res = []
    for strided in (False, True):
        L = Layout(strided)
        res.append(run(L))
        L.check()
    assert len(res[0]) == len(res[1])
    for i, (x, y) in enumerate(zip(*res)):
        same_bits(x, y, f"result {i}, contiguous vs strided")
    return res[0]


def launches(family, fn):
    """how many launches of a timing family one call makes (timing on around this call only)"""
    ops.timing_enable(True)
    try:
        ops.timing_reset()
        fn()
        torch.cuda.synchronize()
        return ops.timing_get(family)[0]
    finally:
        ops.timing_enable(False)


@functools.lru_cache(maxsize=2)
def operands(M, N, K, dtype, seed):
    """A [M,K], W [N,K] (rounded to the compute dtype), bias [N]: numpy fp32.  Computed once per shape and left unchanged."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((M, K), dtype=np.float32)
    w = rng.standard_normal((N, K), dtype=np.float32) * np.float32(K ** -0.5)
    b = rng.standard_normal(N, dtype=np.float32)
    if dtype == BF16:
        a, w = bf16_round(a), bf16_round(w)
    return a, w, b


def f64(x):
    return np.asarray(x, dtype=np.float64)


@functools.lru_cache(maxsize=2)
def product64(M, N, K, dtype, seed):
    """A . W^T + bias of operands(...) in float64, computed once per shape and left unchanged"""
    a, w, b = operands(M, N, K, dtype, seed)
    return f64(a) @ f64(w).T + b


def streamed_rows():
    """rows of a 256x256 GEMM with N = 1024 that has more tiles than gemm256.hip's persistent grid (256 workgroups) and than the
    device has CUs: at least one workgroup computes a second tile"""
    return 256 * (max(ops.device_info(0)["cu_count"], 256) // 4 + 1)


SHAPES = {
    "f32-128x128": (F32, 300, 200, 128),
    "bf16-128x128-2stage": (BF16, 300, 200, 128),
    "bf16-128x128-4stage": (BF16, 300, 200, 256),
    "bf16-256x256-2k": (BF16, 6144, 1024, 128),
    "bf16-256x256-3k": (BF16, 6144, 1024, 192),
    "bf16-256x256-streamed": (BF16, None, 1024, 128),
    "bf16-256x256-residual": (BF16, 6144, 1024, 1024),
    "bf16-256x256-residual-streamed": (BF16, None, 1024, 1024),
    "bf16-2b": (BF16, 12288, 512, 64),
    "bf16-2b-n384": (BF16, 16384, 384, 512),
    "fold-128x128-2stage": (BF16, 256, 256, 128),
    "fold-128x128-4stage": (BF16, 256, 256, 256),
    "fold-256x256": (BF16, 8448, 1024, 128),
}


def shape(route):
    dtype, M, N, K = SHAPES[route]
    return dtype, (streamed_rows() if M is None else M), N, K


def test_shapes_stay_inside_the_32_bit_offsets_the_routes_are_chosen_under():
    """the dispatch does not depend on a leading dimension as long as M * lda * 2 and N * ldw * 2 stay below 2^31"""
    for route in SHAPES:
        _, M, N, K = shape(route)
        assert M * F.default_ld(K) * 2 < 2 ** 31 and N * F.default_ld(K) * 2 < 2 ** 31, route


# ---------------------------------------------------------------------------------------------------------------------------------
# plain epilogue: bias, f32 or compute-dtype out (lda, ldw, ldo)
# ---------------------------------------------------------------------------------------------------------------------------------
PLAIN = [("f32-128x128", F32), ("bf16-128x128-2stage", F32), ("bf16-128x128-2stage", BF16), ("bf16-128x128-4stage", F32),
         ("bf16-128x128-4stage", BF16), ("bf16-256x256-2k", F32), ("bf16-256x256-2k", BF16), ("bf16-256x256-3k", BF16),
         ("bf16-256x256-streamed", F32), ("bf16-256x256-streamed", BF16)]
# (the two-workgroup kernel never takes a GEMM without a residual: gemm.hip use2b)


@pytest.mark.parametrize("route,out_dtype", PLAIN, ids=[f"{r}-{'f32out' if o == F32 else 'bf16out'}" for r, o in PLAIN])
def test_gemm_bias(route, out_dtype):
    dtype, M, N, K = shape(route)
    a, w, b = operands(M, N, K, dtype, 1)
    A, W, Bv = t(a, TDT[dtype]), t(w, TDT[dtype]), t(b)

    def run(L):
        fa, fw, fb = L.inp(A), L.inp(W), L.flat(Bv)
        fo = L.out(M, N, TDT[out_dtype])
        call("pmhip_gemm", dtype, fa, fa.ld, fw, fw.ld, fb, None, 0, 0, fo, fo.ld, out_dtype, M, N, K)
        return [fo.payload()]

    (out,) = both(run)
    ref = product64(M, N, K, dtype, 1)
    assert rel_err(n(out), ref) < (2e-5 if out_dtype == F32 else 1e-2), rel_err(n(out), ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# f32 residual (ldr), with and without the row modulo, and in place (out == residual)
# ---------------------------------------------------------------------------------------------------------------------------------
RESIDUAL = ["f32-128x128", "bf16-128x128-2stage", "bf16-128x128-4stage", "bf16-256x256-residual", "bf16-256x256-residual-streamed",
            "bf16-2b", "bf16-2b-n384"]


@pytest.mark.parametrize("route", RESIDUAL)
def test_gemm_f32_residual_modulo_and_in_place(route):
    dtype, M, N, K = shape(route)
    a, w, b = operands(M, N, K, dtype, 2)
    rows = 16 if M < 1024 else 1024
    r = np.random.default_rng(3).standard_normal((M, N), dtype=np.float32)
    A, W, Bv, R = t(a, TDT[dtype]), t(w, TDT[dtype]), t(b), t(r)
    POS = R[:rows].contiguous()

    def run(L, res, res_rows, in_place=False):
        fa, fw, fb = L.inp(A), L.inp(W), L.flat(Bv)
        if in_place:
            fo = fr = L.out(M, N, f32, payload=res)
        else:
            fr, fo = L.inp(res), L.out(M, N, f32)
        call("pmhip_gemm", dtype, fa, fa.ld, fw, fw.ld, fb, fr, fr.ld, res_rows, fo, fo.ld, F32, M, N, K)
        return [fo.payload()]

    (full,) = both(lambda L: run(L, R, 0))
    (inpl,) = both(lambda L: run(L, R, 0, in_place=True))
    same_bits(inpl, full, "in place vs out of place")
    (mod,) = both(lambda L: run(L, POS, rows))
    ref = product64(M, N, K, dtype, 2)
    assert rel_err(n(full), ref + r) < 2e-5 and rel_err(n(mod), ref + r[np.arange(M) % rows]) < 2e-5
    # the route: only the 2b shapes reach the two-workgroups-per-CU kernel
    assert launches("gemm_resid2b", lambda: run(Layout(True), R, 0)) == (1 if "2b" in route else 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the bf16 pair producers (pmhip_gemm_hilo, _stats, _center): ldr, ldo, row_stats, shift; in place like the engine runs them
# ---------------------------------------------------------------------------------------------------------------------------------
PAIR = ["bf16-128x128-2stage", "bf16-128x128-4stage", "bf16-256x256-residual", "bf16-256x256-residual-streamed", "bf16-2b", "bf16-2b-n384"]
# (f32 operands have no pair producer: gemm_hilo_impl is bf16 only)


def _pair_setup(route, with_stats, seed):
    dtype, M, N, K = shape(route)
    if with_stats:
        N = N // 64 * 64                                            # row_stats: N a multiple of 64 (200 -> 192 on the ragged routes)
    a, w, b = operands(M, N, K, dtype, seed)
    res = np.random.default_rng(seed + 1).standard_normal((M, N), dtype=np.float32) * 1.5 + 30.0
    rh, rl = ops.split_hilo(t(res))
    return M, N, K, a, w, b, t(a, bf16), t(w, bf16), t(b), rh, rl


def _pair_call(L, variant, A, W, Bv, rh, rl, res_rows, M, N, K, in_place=False, coef=None, shift0=None):
    """variant: plain | stats | center1 (centre, shift <- 0) | center2 (centre, statistics when N % 64 == 0, shift += c)"""
    fa, fw, fb = L.inp(A), L.inp(W), L.flat(Bv)
    if in_place:
        oh = frh = L.out(M, N, bf16, payload=rh)
        ol = frl = L.out(M, N, bf16, payload=rl)
    else:
        frh, frl = L.inp(rh), L.inp(rl)
        oh, ol = L.out(M, N, bf16), L.out(M, N, bf16)
    assert frh.ld == frl.ld and oh.ld == ol.ld
    head = (fa, fa.ld, fw, fw.ld, fb, frh, frl, frh.ld, res_rows, oh, ol, oh.ld, M, N, K)
    res = [oh, ol]
    if variant == "plain":
        call("pmhip_gemm_hilo", *head)
    elif variant == "stats":
        st = L.out(M, N // 64 * 2, f32, flat=True)
        call("pmhip_gemm_hilo_stats", *head, st)
        res.append(st)
    else:
        st = L.out(M, N // 64 * 2, f32, flat=True) if (variant == "center2" and N % 64 == 0) else None
        sh = L.out(M, 1, f32, payload=shift0, flat=True)
        call("pmhip_gemm_hilo_center", *head, st, L.flat(coef), 0.25, sh, 1 if variant == "center1" else 2)
        res += [sh] + ([st] if st is not None else [])
    return [f.payload() for f in res]


@pytest.mark.parametrize("route", PAIR)
@pytest.mark.parametrize("variant", ["plain", "stats", "center1", "center2"])
def test_gemm_hilo_pair(route, variant):
    M, N, K, a, w, b, A, W, Bv, rh, rl = _pair_setup(route, variant in ("stats", "center2"), 4)
    coef = ops.ln_coef(rh) if variant.startswith("center") else None
    shift0 = torch.full((M, 1), 7.0, device=dev()) if coef is not None else None
    kw = dict(coef=coef, shift0=shift0)
    out = both(lambda L: _pair_call(L, variant, A, W, Bv, rh, rl, 0, M, N, K, **kw))
    inpl = both(lambda L: _pair_call(L, variant, A, W, Bv, rh, rl, 0, M, N, K, in_place=True, **kw))
    for i, (x, y) in enumerate(zip(inpl, out)):
        same_bits(x, y, f"result {i}, in place vs out of place")
    # float64, as tests/test_gpu_ops.py does for the producers
    r64 = f64(n(ops.join_hilo(rh, rl)))
    want = product64(M, N, K, BF16, 4) + r64
    got = f64(n(out[0])) + f64(n(out[1]))
    if variant in ("plain", "stats"):
        assert np.max(np.abs(got - want)) < 2e-5 * max(1.0, np.abs(want).max()), np.max(np.abs(got - want))
    else:
        c = n(coef).astype(np.float64)
        cen = 0.25 - c[:, 1] / c[:, 0]
        sh = f64(n(out[2]))[:, 0]
        assert np.abs(sh - (0.0 if variant == "center1" else 7.0 + cen)).max() < 1e-4       # shift <- 0 / shift += c
        assert np.max(np.abs(got + cen[:, None] - want)) < 3e-5 * max(1.0, np.abs(want - cen[:, None]).max())
    if variant == "stats":
        h64 = f64(n(out[0])).reshape(M, N // 64, 64)
        p = n(out[2]).reshape(M, N // 64, 2)
        assert np.abs(p[..., 0] - h64.sum(-1)).max() < 2e-4
        assert np.abs(p[..., 1] - ((h64 - h64.mean(-1, keepdims=True)) ** 2).sum(-1)).max() < 2e-3
    if variant == "plain":                                           # the row modulo (a position-embedding pair) and the route
        rows = 16 if M < 1024 else 1024
        ph, pl = rh[:rows].contiguous(), rl[:rows].contiguous()
        mod = both(lambda L: _pair_call(L, "plain", A, W, Bv, ph, pl, rows, M, N, K))
        want = product64(M, N, K, BF16, 4) + r64[np.arange(M) % rows]
        got = f64(n(mod[0])) + f64(n(mod[1]))
        assert np.max(np.abs(got - want)) < 2e-5 * max(1.0, np.abs(want).max())
        took2b = launches("gemm_resid2b", lambda: _pair_call(Layout(True), "plain", A, W, Bv, rh, rl, 0, M, N, K))
        assert took2b == (1 if "2b" in route else 0)


@pytest.mark.parametrize("route", PAIR)
def test_gemm_hilo_center_in_place_twice_accumulates_the_shift(route):
    """The engine's pattern: every residual producer of a layer runs in place on the same pair and adds what it subtracted to the
    same `shift`.  Two producers in a row, in place, against the same two producers writing fresh planes."""
    M, N, K, a, w, b, A, W, Bv, rh, rl = _pair_setup(route, True, 6)
    coef = ops.ln_coef(rh)

    def run(L, in_place):
        fa, fw, fb, fc = L.inp(A), L.inp(W), L.flat(Bv), L.flat(coef)
        sh = L.out(M, 1, f32, payload=torch.zeros(M, 1, device=dev()), flat=True)
        if in_place:
            planes = [(L.out(M, N, bf16, payload=rh), L.out(M, N, bf16, payload=rl))] * 3
        else:
            planes = [(L.inp(rh), L.inp(rl))] + [(L.out(M, N, bf16), L.out(M, N, bf16)) for _ in range(2)]
        for (ih, il), (oh, ol) in zip(planes[:2], planes[1:]):
            st = L.out(M, N // 64 * 2, f32, flat=True)
            call("pmhip_gemm_hilo_center", fa, fa.ld, fw, fw.ld, fb, ih, il, ih.ld, 0, oh, ol, oh.ld, M, N, K, st, fc, 0.25, sh, 2)
        return [planes[2][0].payload(), planes[2][1].payload(), sh.payload(), st.payload()]

    fresh = both(lambda L: run(L, False))
    inpl = both(lambda L: run(L, True))
    for i, (x, y) in enumerate(zip(inpl, fresh)):
        same_bits(x, y, f"result {i}, in place vs fresh planes")
    c = n(coef).astype(np.float64)
    assert np.abs(f64(n(fresh[2]))[:, 0] - 2 * (0.25 - c[:, 1] / c[:, 0])).max() < 2e-4      # two producers, two subtractions


# ---------------------------------------------------------------------------------------------------------------------------------
# SwiGLU (lda, ldo; W12p is packed and has no leading dimension)
# ---------------------------------------------------------------------------------------------------------------------------------
# N = 2 * Hp.  The two-workgroup kernel never takes a SwiGLU GEMM (use2b: plain epilogue with a residual only); an f32 result exists
# on the f32 route only (launch_bf16).
SWIGLU = {"f32-128x128": (F32, 300, 128, 128), "bf16-128x128-2stage": (BF16, 300, 128, 128), "bf16-128x128-4stage": (BF16, 300, 128, 256),
          "bf16-256x256-2k": (BF16, 6144, 512, 128), "bf16-256x256-streamed": (BF16, None, 512, 128)}


def _swiglu_ref(a, w12p, b12p, Hp):
    x12 = (f64(a) @ f64(w12p).T + b12p).reshape(a.shape[0], Hp // 16, 2, 16)     # packed rows: 16 of x1, the matching 16 of x2, ...
    x1, x2 = x12[:, :, 0].reshape(-1, Hp), x12[:, :, 1].reshape(-1, Hp)
    return x1 / (1.0 + np.exp(-x1)) * x2


@pytest.mark.parametrize("route", list(SWIGLU))
def test_gemm_swiglu(route):
    dtype, M, Hp, K = SWIGLU[route]
    M = streamed_rows() if M is None else M
    a, w, b = operands(M, 2 * Hp, K, dtype, 7)
    A, W, Bv = t(a, TDT[dtype]), t(w, TDT[dtype]), t(b)

    def run(L):
        fa, fo = L.inp(A), L.out(M, Hp, TDT[dtype])
        call("pmhip_gemm_swiglu", dtype, fa, fa.ld, L.flat(W), L.flat(Bv), fo, fo.ld, M, Hp, K)
        return [fo.payload()]

    (out,) = both(run)
    assert rel_err(n(out), _swiglu_ref(a, w, b, Hp)) < (2e-5 if dtype == F32 else 2e-2)


# ---------------------------------------------------------------------------------------------------------------------------------
# head split (lda, ldw): Q, K and V^T prefilled with the sentinel; the padding [tokens, tokens_pad) of K / V^T stays untouched
# ---------------------------------------------------------------------------------------------------------------------------------
# ragged routes: 3 images; the 256x256 route needs M = B * tokens a multiple of 256 and >= 96 tiles (N = 3 * 4 * 64 = 768: 3 tile columns)
# streamed: eight heads instead of four double the tile columns (462 / 300 tiles: more than the persistent grid's 256 workgroups)
HEADS = {"f32-128x128": (F32, 3, 128), "bf16-128x128-2stage": (BF16, 3, 128), "bf16-128x128-4stage": (BF16, 3, 256),
         "bf16-256x256-2k": (BF16, None, 128), "bf16-256x256-streamed": (BF16, None, 128)}
# (the two-workgroup kernel never takes a head-split GEMM: use2b)


def _heads_outs(L, kinds, B, heads, dh, tokens, tp, dtype):
    outs = []
    for kind in kinds:
        rows, cols = (B * heads * tokens, dh) if kind == PART_Q else ((B * heads * tp, dh) if kind == PART_K else (B * heads * dh, tp))
        outs.append(L.out(rows, cols, dtype, flat=True))
    return outs


def _heads_check(kinds, got, full, B, heads, dh, tokens, tp, dtype, q_scale, tol):
    """got: the flat payloads; full: float64 [B, tokens, nparts, heads, dh].  Values against float64; the padding of K / V^T must
    still hold the sentinel (include/pmhip.h: every route leaves it alone)."""
    sentinel = F._BITS[dtype][1]
    for i, kind in enumerate(kinds):
        x = got[i]
        if kind == PART_Q:
            assert rel_err(n(x).reshape(B, heads, tokens, dh), full[:, :, i].transpose(0, 2, 1, 3) * q_scale) < tol
        elif kind == PART_K:
            x = x.reshape(B, heads, tp, dh)
            assert rel_err(n(x[:, :, :tokens]), full[:, :, i].transpose(0, 2, 1, 3)) < tol
            assert bool((bits(x[:, :, tokens:]) == sentinel).all()), "K padding rows were written"
        else:
            x = x.reshape(B, heads, dh, tp)
            assert rel_err(n(x[..., :tokens]), full[:, :, i].transpose(0, 2, 3, 1)) < tol
            assert bool((bits(x[..., tokens:]) == sentinel).all()), "V^T padding columns were written"


@pytest.mark.parametrize("tokens", [77, 200])
@pytest.mark.parametrize("route", list(HEADS))
def test_gemm_heads(route, tokens):
    dtype, B, K = HEADS[route]
    heads, kinds = (8 if route.endswith("streamed") else 4), [PART_Q, PART_K, PART_V]
    if B is None:
        B = {77: 256, 200: 64}[tokens]                              # 77 x 256 / 50 x 256 rows: 231 / 150 tiles with four heads, 462 / 300 with eight
    M, N, tp = B * tokens, 3 * heads * 64, (tokens + 63) // 64 * 64
    assert tp > tokens
    a, w, _ = operands(M, N, K, dtype, 8)
    A, W = t(a, TDT[dtype]), t(w, TDT[dtype])
    kinds_c = (C.c_int * 3)(*kinds)

    def run(L):
        fa, fw = L.inp(A), L.inp(W)
        outs = _heads_outs(L, kinds, B, heads, 64, tokens, tp, TDT[dtype])
        outs_c = (C.c_void_p * 3)(*[o.ptr for o in outs])
        call("pmhip_gemm_heads", dtype, fa, fa.ld, fw, fw.ld, M, K, heads, tokens, tp, 3, kinds_c, outs_c, 0.125)
        return [o.payload() for o in outs]

    got = both(run)
    full = (f64(a) @ f64(w).T).reshape(B, tokens, 3, heads, 64)
    _heads_check(kinds, got, full, B, heads, 64, tokens, tp, TDT[dtype], 0.125, 2e-5 if dtype == F32 else 1e-2)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_gemm_heads_dh32(dtype):
    """dim_head != 64: an ordinary GEMM into the caller's f32 scratch, then the split kernel"""
    B, heads, dh, tokens, K = 3, 4, 32, 77, 128
    kinds = [PART_Q, PART_K, PART_V]
    M, N, tp = B * tokens, 3 * heads * dh, 128
    a, w, _ = operands(M, N, K, dtype, 9)
    A, W = t(a, TDT[dtype]), t(w, TDT[dtype])
    kinds_c = (C.c_int * 3)(*kinds)

    def run(L):
        fa, fw = L.inp(A), L.inp(W)
        outs = _heads_outs(L, kinds, B, heads, dh, tokens, tp, TDT[dtype])
        scratch = L.out(M, N, f32, flat=True)
        outs_c = (C.c_void_p * 3)(*[o.ptr for o in outs])
        call("pmhip_gemm_heads_dh", dtype, fa, fa.ld, fw, fw.ld, M, K, heads, dh, tokens, tp, 3, kinds_c, outs_c, 0.125, scratch)
        return [o.payload() for o in outs]

    got = both(run)
    full = (f64(a) @ f64(w).T).reshape(B, tokens, 3, heads, dh)
    _heads_check(kinds, got, full, B, heads, dh, tokens, tp, TDT[dtype], 0.125, 2e-5 if dtype == F32 else 1e-2)


# ---------------------------------------------------------------------------------------------------------------------------------
# the logits GEMM with the sampler's block statistics (ldo; block_stats framed)
# ---------------------------------------------------------------------------------------------------------------------------------
# N % 64 == 0: 192 columns on the ragged routes.  No residual, so never the two-workgroup kernel.
STATS = {"f32-128x128": (F32, 300, 192, 128), "bf16-128x128-2stage": (BF16, 300, 192, 128), "bf16-128x128-4stage": (BF16, 300, 192, 256),
         "bf16-256x256-2k": (BF16, 6144, 1024, 128)}


@pytest.mark.parametrize("route", list(STATS))
def test_gemm_softmax_stats(route):
    dtype, M, N, K = STATS[route]
    a, w, b = operands(M, N, K, dtype, 10)
    A, W, Bv = t(a, TDT[dtype]), t(w, TDT[dtype]), t(b)

    def run(L):
        fa, fw, fb = L.inp(A), L.inp(W), L.flat(Bv)
        fo, fs = L.out(M, N, f32), L.out(M, N // 64 * 2, f32, flat=True)
        call("pmhip_gemm_softmax_stats", dtype, fa, fa.ld, fw, fw.ld, fb, fo, fo.ld, M, N, K, None, fs)
        return [fo.payload(), fs.payload()]

    logits, stats = both(run)
    assert rel_err(n(logits), product64(M, N, K, dtype, 10)) < 2e-5
    same_bits(logits, ops.gemm(A, W, bias=Bv, out_dtype=f32), "logits vs the plain call")
    _, want = ops.guidance_combine(logits, logits, 1.0, with_stats=True)      # the statistics of what is stored, same arithmetic
    same_bits(stats.reshape(M, N // 64, 2), want, "block statistics")


# ---------------------------------------------------------------------------------------------------------------------------------
# folded LayerNorm consumers: plain / SwiGLU / head split / logits with statistics, on the three folded routes
# ---------------------------------------------------------------------------------------------------------------------------------
FOLD = ["fold-128x128-2stage", "fold-128x128-4stage", "fold-256x256"]


def _fold_setup(route, seed):
    _, M, N, K = shape(route)
    rng = np.random.default_rng(seed)
    hi = t(rng.standard_normal((M, K), dtype=np.float32) + 0.4, bf16)
    wg = bf16_round(rng.standard_normal((N, K), dtype=np.float32) * np.float32(K ** -0.5))
    b, d = rng.standard_normal(N, dtype=np.float32), 0.2 * rng.standard_normal(N, dtype=np.float32)
    c = wg.sum(1, dtype=np.float32)
    h = hi.float().reshape(M, K // 64, 64)                          # the producer's partial statistics of this hi plane
    s = h.sum(-1)
    parts = torch.stack([s, ((h - s[..., None] / 64) ** 2).sum(-1)], -1).contiguous()
    coef = ops.ln_coef_parts(parts)                                 # the coefficients both forms must use, bit for bit
    h64 = f64(n(hi))
    rstd = 1.0 / np.sqrt(h64.var(1) + 1e-5)
    y64 = (rstd[:, None] * (h64 @ f64(wg).T) - (rstd * h64.mean(1))[:, None] * f64(c) + d)     # = LN(hi) . W^T with gamma, beta folded
    return M, N, K, hi, t(wg, bf16), t(b), t(c), t(d), parts, coef, y64, b


def _lnfold(L, coef, c, d, parts, K, from_parts):
    """-> (descriptor, the coef frame when it is an OUTPUT of the call)"""
    ln = _lib.LnFold()
    fc, fd = L.flat(c), L.flat(d)
    if from_parts:
        fcoef, fp = L.out(coef.shape[0], 2, f32, flat=True), L.flat(parts)
        ln.parts, ln.nparts, ln.eps = fp.ptr, K // 64, 1e-5
    else:
        fcoef, fp = L.flat(coef), None
    ln.coef, ln.c, ln.d = fcoef.ptr, fc.ptr, fd.ptr
    ln._keep = (fcoef, fc, fd, fp)
    return ln, (fcoef if from_parts else None)


def _fold_both(body, make_ln, coef):
    """body(L, lnfold) -> results; make_ln(L, from_parts) -> _lnfold(...).  Coefficients given, then derived from `parts` by the
    call (the GEMM's prologue on the four-stage small route, pmhip_ln_coef_parts launched by the call elsewhere): same results,
    and coef written equal to `coef`."""
    def run(L, from_parts):
        ln, fcoef = make_ln(L, from_parts)
        res = body(L, ln)
        return res + ([fcoef.payload()] if fcoef is not None else [])

    given = both(lambda L: run(L, False))
    derived = both(lambda L: run(L, True))
    for i, x in enumerate(given):
        same_bits(derived[i], x, f"result {i}, coef from parts vs coef given")
    same_bits(derived[-1], coef, "coef written by the call vs pmhip_ln_coef_parts")
    return given


@pytest.mark.parametrize("epi", ["plain-f32out", "plain-bf16out", "swiglu", "heads", "softmax-stats"])
@pytest.mark.parametrize("route", FOLD)
def test_gemm_folded_layernorm(route, epi):
    M, N, K, hi, W, Bv, c, d, parts, coef, y64, b = _fold_setup(route, 11)
    heads, tokens, kinds = N // 128, 128, [PART_K, PART_V]          # head split: N = 2 parts x heads x 64, M a multiple of 128 tokens
    kinds_c = (C.c_int * 2)(*kinds)

    def body(L, ln):
        fa = L.inp(hi)
        if epi.startswith("plain"):
            fw, od = L.inp(W), (F32 if epi == "plain-f32out" else BF16)
            fo = L.out(M, N, TDT[od])
            call("pmhip_gemm_ln", BF16, fa, fa.ld, fw, fw.ld, L.flat(Bv), fo, fo.ld, od, M, N, K, C.byref(ln))
            return [fo.payload()]
        if epi == "swiglu":
            fo = L.out(M, N // 2, bf16)
            call("pmhip_gemm_swiglu_ln", BF16, fa, fa.ld, L.flat(W), L.flat(Bv), fo, fo.ld, M, N // 2, K, C.byref(ln))
            return [fo.payload()]
        if epi == "heads":
            fw = L.inp(W)
            outs = _heads_outs(L, kinds, M // tokens, heads, 64, tokens, tokens, bf16)
            outs_c = (C.c_void_p * 2)(*[o.ptr for o in outs])
            call("pmhip_gemm_heads_ln", BF16, fa, fa.ld, fw, fw.ld, M, K, heads, tokens, tokens, 2, kinds_c, outs_c, 1.0, C.byref(ln))
            return [o.payload() for o in outs]
        fw = L.inp(W)
        fo, fs = L.out(M, N, f32), L.out(M, N // 64 * 2, f32, flat=True)
        call("pmhip_gemm_softmax_stats", BF16, fa, fa.ld, fw, fw.ld, L.flat(Bv), fo, fo.ld, M, N, K, C.byref(ln), fs)
        return [fo.payload(), fs.payload()]

    got = _fold_both(body, lambda L, from_parts: _lnfold(L, coef, c, d, parts, K, from_parts), coef)
    if epi.startswith("plain"):
        assert rel_err(n(got[0]), y64 + b) < 2e-2
    elif epi == "swiglu":
        x12 = (y64 + b).reshape(M, N // 32, 2, 16)
        x1, x2 = x12[:, :, 0].reshape(M, -1), x12[:, :, 1].reshape(M, -1)
        assert rel_err(n(got[0]), x1 / (1.0 + np.exp(-x1)) * x2) < 3e-2
    elif epi == "heads":
        full = y64.reshape(M // tokens, tokens, 2, heads, 64)
        _heads_check(kinds, got, full, M // tokens, heads, 64, tokens, tokens, bf16, 1.0, 2e-2)
    else:
        assert rel_err(n(got[0]), y64 + b) < 2e-2
        _, want = ops.guidance_combine(got[0], got[0], 1.0, with_stats=True)
        same_bits(got[1].reshape(M, N // 64, 2), want, "block statistics")


# ---------------------------------------------------------------------------------------------------------------------------------
# attention: ldo = heads * dh + 72, out and Q framed, NaN in the K / V^T padding
# ---------------------------------------------------------------------------------------------------------------------------------
def _attention_case(dtype, B, H, dh, Nq, Nkv, entry):
    tdt, fast = TDT[dtype], dtype == BF16
    Nkp = (Nkv + 63) // 64 * 64
    rng = np.random.default_rng(B * 1000 + Nq + Nkv + dh)
    rd = lambda *s: rng.standard_normal(s, dtype=np.float32)
    q, k, v = rd(B, H, Nq, dh) * np.float32(dh ** -0.5), rd(B, H, Nkp, dh), rd(B, H, Nkp, dh)
    if fast:
        q, k, v = bf16_round(q), bf16_round(k), bf16_round(v)
    kp, vtp = k.copy(), np.ascontiguousarray(v.transpose(0, 1, 3, 2))
    kp[:, :, Nkv:] = np.nan                                        # the padding may hold anything
    vtp[..., Nkv:] = np.nan
    Q = t(q * np.float32(ops.LOG2E) if fast else q, tdt)            # use_exp2: Q carries the extra log2(e)
    Kt, Vt = t(kp, tdt), t(vtp, tdt)

    def run(L):
        fo = L.out(B * Nq, H * dh, tdt, ld=H * dh + 72)
        args = (dtype, L.flat(Q), L.flat(Kt), L.flat(Vt), fo, fo.ld, B, H)
        if entry == "pmhip_attention":
            call(entry, *args, Nq, Nkv, Nkp, int(fast))
        else:
            call(entry, *args, dh, Nq, Nkv, Nkp, int(fast))
        return [fo.payload()]

    (out,) = both(run)
    q_eff = f64(n(Q)) / (ops.LOG2E if fast else 1.0)
    s = q_eff @ f64(k[:, :, :Nkv]).transpose(0, 1, 3, 2)
    p = np.exp(s - s.max(-1, keepdims=True))
    ref = ((p / p.sum(-1, keepdims=True)) @ f64(v[:, :, :Nkv])).transpose(0, 2, 1, 3).reshape(B * Nq, H * dh)
    assert np.isfinite(n(out)).all() and rel_err(n(out), ref) < (3e-5 if dtype == F32 else 3e-2), rel_err(n(out), ref)


# the bf16 kernel serves 256 / 128 / 64 queries per workgroup (attention_bf16.hip pm_attention_bf16: 256 while B * heads *
# ceil(Nq / 256) >= 512, 128 while B * heads * ceil(Nq / 128) >= 512, else 64); Nq = 77 has one tile either way, so 128 queries
# per workgroup exist at Nq = 200 only.  Nq = 77 / 200: the last query tile is ragged inside EVERY image.
ATTN = [("f32", F32, 2, 3, 77), ("f32", F32, 2, 3, 200), ("bf16-64q", BF16, 2, 3, 77), ("bf16-64q", BF16, 2, 3, 200),
        ("bf16-128q", BF16, 32, 8, 200), ("bf16-256q", BF16, 64, 8, 77), ("bf16-256q", BF16, 64, 8, 200)]


@pytest.mark.parametrize("Nkv", [77, 130])
@pytest.mark.parametrize("kernel,dtype,B,H,Nq", ATTN, ids=[f"{k}-B{b}H{h}-Nq{q}" for k, _, b, h, q in ATTN])
def test_attention(kernel, dtype, B, H, Nq, Nkv):
    _attention_case(dtype, B, H, 64, Nq, Nkv, "pmhip_attention")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("dh,H", [(32, 2), (128, 3)])
def test_attention_dh(dh, H, dtype):
    _attention_case(dtype, 2, H, dh, 77, 130, "pmhip_attention_dh")


# ---------------------------------------------------------------------------------------------------------------------------------
# samplers and loss: ldl = V + 72, NaN in the gap and in the guard rows; pred, ids_out, score, row_loss framed
# ---------------------------------------------------------------------------------------------------------------------------------
def _sample_inputs(M, V, seed):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((M, V)) * 2.0).astype(np.float32)
    ids = rng.integers(0, V, M).astype(np.int64)
    ids[rng.random(M) < 0.6] = V
    noise = rng.random((M, V)).astype(np.float32)
    return logits, ids, noise


def _sample_outs(L, M):
    return [L.out(M, 1, i64, flat=True), L.out(M, 1, i64, flat=True), L.out(M, 1, f32, flat=True)]


@pytest.mark.parametrize("kernel,V,topk,stats", [("dense", 1000, 16, False), ("blocks", 1024, 5, False), ("blocks", 1024, 5, True)],
                         ids=["dense-V1000-top16", "blocks-V1024-top5", "blocks-V1024-top5-stats-given"])
def test_sample_rows(kernel, V, topk, stats):
    M = 300
    logits, ids, noise = _sample_inputs(M, V, V + topk)
    X, I, NZ = t(logits), t(ids), t(noise)
    st = ops.guidance_combine(X, X, 1.0, with_stats=True)[1] if stats else None

    def run(L, nz):
        fx = L.inp(X, ld=V + 72)
        outs = _sample_outs(L, M)
        tail = (L.flat(I), V, topk, 0.8, (L.flat(nz) if nz is not None else None), 77, 3, 1234, *outs, M, V)
        if stats:
            call("pmhip_sample_rows_stats", fx, fx.ld, L.flat(st), *tail)
        else:
            call("pmhip_sample_rows", fx, fx.ld, *tail)
        return [o.payload().reshape(M) for o in outs]

    pred, merged, score = both(lambda L: run(L, NZ))
    pred_r, merged_r, score_r = O.sample_rows(logits, ids, V, topk, 0.8, noise)
    assert np.array_equal(n(pred), pred_r) and np.array_equal(n(merged), merged_r) and np.max(np.abs(n(score) - score_r)) < 2e-6
    philox = both(lambda L: run(L, None))                           # counter-based noise: the same draws in either layout
    for got, want in zip(philox, ops.sample_rows(X, I, V, topk, 0.8, seed=77, step=3, row_base=1234, block_stats=st)):
        same_bits(got, want, "Philox draw vs paintmind_amd.ops")


@pytest.mark.parametrize("stats", [False, True], ids=["stats-derived", "stats-given"])
def test_sample_rows_slots_with_an_idle_slot(stats):
    V, tokens, recs = 1024, 100, [(0x0123456789ABCDEF, 7, 0.0, 1, 1, 0), None, (77, 2 ** 33 + 5, 0.8, 8, 50, 3)]
    M = tokens * len(recs)
    logits, ids, _ = _sample_inputs(M, V, 5)
    X, I = t(logits), t(ids)
    st = ops.guidance_combine(X, X, 1.0, with_stats=True)[1] if stats else None
    slots = ops.pack_slots(recs, dev())

    def run(L):
        fx = L.inp(X, ld=V + 72)
        outs = _sample_outs(L, M)
        call("pmhip_sample_rows_slots", fx, fx.ld, (L.flat(st) if stats else None), L.flat(I), V, L.flat(slots), tokens, *outs, M, V)
        return [o.payload().reshape(M) for o in outs]

    pred, merged, score = both(run)
    for b, rec in enumerate(recs):                                   # include/pmhip.h: image b equals the scalar entry on its rows alone
        r = slice(b * tokens, (b + 1) * tokens)
        if rec is None:
            assert torch.equal(pred[r], I[r]) and torch.equal(merged[r], I[r]) and bool((score[r] == -1e5).all())
            continue
        seed, k, temp, topk, _, step = rec
        one = ops.sample_rows(X[r].contiguous(), I[r].contiguous(), V, topk, temp, seed=seed, step=step, row_base=k * tokens)
        for got, want in zip((pred[r], merged[r], score[r]), one):
            same_bits(got.contiguous(), want, f"image {b} vs the scalar entry")
        cols = np.broadcast_to(np.arange(V), (tokens, V))
        rows = np.broadcast_to((np.uint64(k) * np.uint64(tokens) + np.arange(tokens, dtype=np.uint64))[:, None], (tokens, V))
        pred_r, merged_r, score_r = O.sample_rows(logits[r], ids[r], V, topk, temp, O.philox_uniform(seed, step, rows, cols))
        assert np.array_equal(n(pred[r]), pred_r) and np.array_equal(n(merged[r]), merged_r)
        assert np.max(np.abs(n(score[r]) - score_r)) < 2e-6


@pytest.mark.parametrize("M,V,eps", [(300, 1000, 0.0), (17, 8200, 0.3)])
def test_masked_ce(M, V, eps):
    rng = np.random.default_rng(M + V)
    logits = (rng.standard_normal((M, V)) * 4).astype(np.float32)
    labels = rng.integers(0, V, M)
    mask = (rng.random(M) < 0.5).astype(np.float32)
    X, Y, Mk = t(logits), t(labels), t(mask)

    def run(L):
        fx = L.inp(X, ld=V + 72)
        rows, loss = L.out(M, 1, f32, flat=True), L.out(1, 1, f32, flat=True)
        call("pmhip_masked_ce", fx, fx.ld, L.flat(Y), L.flat(Mk), eps, rows, loss, M, V)
        return [rows.payload().reshape(M), loss.payload().reshape(1)]

    rows, loss = both(run)
    lo, ro = O.masked_ce(logits, labels, mask, eps)
    assert maxabs(n(rows), ro) < 1e-4 and abs(float(loss) - float(lo)) < 1e-4


# ---------------------------------------------------------------------------------------------------------------------------------
# row operators and the rest: no leading dimension, so only the bounds half -- framed inputs and outputs, one ragged shape each,
# the result bit-identical to the paintmind_amd.ops call (which tests/test_gpu_ops.py holds against the oracle)
# ---------------------------------------------------------------------------------------------------------------------------------
def rowop(entry, make_args, wants):
    """make_args(L) -> (argument tuple, output frames); `wants`: the tensors paintmind_amd.ops returns for the same inputs"""
    L = Layout(False)
    args, outs = make_args(L)
    call(entry, *args)
    L.check()
    assert len(outs) == len(wants)
    for i, (f, want) in enumerate(zip(outs, wants)):
        same_bits(f.payload().reshape(want.shape), want.contiguous(), f"{entry}: output {i} vs paintmind_amd.ops")


def rnd(*shape, scale=1.0, seed=0):
    return t((np.random.default_rng(seed + len(shape)).standard_normal(shape) * scale).astype(np.float32))


@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["f32out", "bf16out"])
def test_rowop_layernorm(out_dtype):
    M, D = 77, 1280
    x, g, b = rnd(M, D, scale=3.0) + 0.5, rnd(D, seed=1) + 1, rnd(D, seed=2)

    def args(L):
        o = L.out(M, D, TDT[out_dtype], flat=True)
        return (L.flat(x), L.flat(g), L.flat(b), 1e-5, o, out_dtype, M, D), [o]
    rowop("pmhip_layernorm", args, [ops.layernorm(x, g, b, 1e-5, TDT[out_dtype])])


def test_rowop_hilo_family():
    M, D = 5, 72
    x, g, b = rnd(M, D, scale=3.0) + 0.9, rnd(D, seed=1) + 1, rnd(D, seed=2)
    hi, lo = ops.split_hilo(x)

    def split(L):
        oh, ol = L.out(M, D, bf16, flat=True), L.out(M, D, bf16, flat=True)
        return (L.flat(x), oh, ol, M, D), [oh, ol]
    rowop("pmhip_split_hilo", split, [hi, lo])

    def join(L):
        o = L.out(M, D, f32, flat=True)
        return (L.flat(hi), L.flat(lo), o, M, D), [o]
    rowop("pmhip_join_hilo", join, [ops.join_hilo(hi, lo)])

    for od in (F32, BF16):
        def ln(L):
            o = L.out(M, D, TDT[od], flat=True)
            return (L.flat(hi), L.flat(lo), L.flat(g), L.flat(b), 1e-5, o, od, M, D), [o]
        rowop("pmhip_layernorm_hilo", ln, [ops.layernorm_hilo(hi, lo, g, b, out_dtype=TDT[od])])

    def to_hilo(L):
        oh, ol = L.out(M, D, bf16, flat=True), L.out(M, D, bf16, flat=True)
        return (L.flat(x), L.flat(g), L.flat(b), 1e-5, oh, ol, M, D), [oh, ol]
    rowop("pmhip_layernorm_to_hilo", to_hilo, list(ops.layernorm_to_hilo(x, g, b)))

    shift = rnd(M, seed=3)

    def unshift(L):                                                  # in place on the pair
        oh, ol = L.out(M, D, bf16, payload=hi, flat=True), L.out(M, D, bf16, payload=lo, flat=True)
        return (oh, ol, L.flat(shift), M, D), [oh, ol]
    rowop("pmhip_unshift_hilo", unshift, list(ops.unshift_hilo(hi.clone(), lo.clone(), shift)))


def test_rowop_ln_coef_and_parts():
    M, D = 77, 192
    hi = rnd(M, D, scale=2.0).to(bf16)

    def coef(L):
        o = L.out(M, 2, f32, flat=True)
        return (L.flat(hi), 1e-5, o, M, D), [o]
    rowop("pmhip_ln_coef", coef, [ops.ln_coef(hi)])
    h = hi.float().reshape(M, 3, 64)
    s = h.sum(-1)
    parts = torch.stack([s, ((h - s[..., None] / 64) ** 2).sum(-1)], -1).contiguous()

    def from_parts(L):
        o = L.out(M, 2, f32, flat=True)
        return (L.flat(parts.reshape(M, 6)), 3, 1e-5, o, M), [o]
    rowop("pmhip_ln_coef_parts", from_parts, [ops.ln_coef_parts(parts)])


def test_rowop_convert_embed_add():
    x = rnd(100, 32)
    for od in (F32, BF16):
        def conv(L):
            o = L.out(100, 64, TDT[od], flat=True)
            return (L.flat(x), 32, o, od, 64, 100), [o]
        rowop("pmhip_convert_pad", conv, [ops.convert_pad(x, 64, TDT[od])])
    table = rnd(65, 32, seed=1)
    ids = t(np.random.default_rng(2).integers(0, 65, 77).astype(np.int64))
    for od in (F32, BF16):
        def emb(L):
            o = L.out(77, 64, TDT[od], flat=True)
            return (L.flat(table), L.flat(ids), o, od, 64, 77, 65, 32), [o]
        rowop("pmhip_embed_rows", emb, [ops.embed_rows(table, ids, 64, TDT[od])])
    xx, pos = rnd(50, 72, seed=3), rnd(16, 72, seed=4)

    def add(L):
        o = L.out(50, 72, f32, flat=True)
        return (L.flat(xx), L.flat(pos), 16, o, 50, 72), [o]
    rowop("pmhip_add_rows", add, [ops.add_rows(xx, pos)])


def test_rowop_patchify_unpatchify():
    B, Cc, S, P = 2, 3, 40, 8                                       # 5 x 5 patches per image
    img = rnd(B, Cc, S, S)
    rows, cols = B * (S // P) ** 2, Cc * P * P
    for od in (F32, BF16):
        def pat(L):
            o = L.out(rows, cols, TDT[od], flat=True)
            return (L.flat(img), o, od, B, Cc, S, S, P), [o]
        rowop("pmhip_patchify", pat, [ops.patchify(img, P, TDT[od])])
    y = rnd(rows, cols, scale=2.0, seed=1)

    def unpat(L):
        o = L.out(B * Cc * S, S, f32, flat=True)
        return (L.flat(y), o, B, Cc, S, S, P, -1.0, 1.0), [o]
    rowop("pmhip_unpatchify_clamp", unpat, [ops.unpatchify_clamp(y, B, Cc, S, P)])


def test_rowop_guidance_combine():
    M, V = 77, 192
    cond, unc = rnd(M, V, scale=2.0), rnd(M, V, scale=2.0, seed=1)

    def plain(L):
        o = L.out(M, V, f32, flat=True)
        return (L.flat(cond), L.flat(unc), 3.0, o, M * V), [o]
    rowop("pmhip_guidance_combine", plain, [ops.guidance_combine(cond, unc, 3.0)])

    def with_stats(L):
        o, s = L.out(M, V, f32, flat=True), L.out(M, V // 64 * 2, f32, flat=True)
        return (L.flat(cond), L.flat(unc), 3.0, o, M * V, s), [o, s]
    rowop("pmhip_guidance_combine_stats", with_stats, list(ops.guidance_combine(cond, unc, 3.0, with_stats=True)))


def test_rowop_remask_and_random_mask():
    B, N, E = 3, 257, 8
    rng = np.random.default_rng(12)
    scores = np.round(rng.random((B, N)).astype(np.float32), 2)     # ties
    scores[:, ::7] = -1e5
    ids = t(rng.integers(0, 50, (B, N)).astype(np.int64))
    S = t(scores)

    def remask(L):                                                   # in place on ids
        o = L.out(B, N, i64, payload=ids, flat=True)
        return (o, L.flat(S), 100, 8192, B, N), [o]
    rowop("pmhip_remask", remask, [ops.remask(ids.clone(), S, 100, 8192)])
    slots = ops.pack_slots([(1, 0, 1.0, 1, 100, 0), None, (2, 1, 1.0, 1, 256, 0)], dev())

    def remask_slots(L):
        o = L.out(B, N, i64, payload=ids, flat=True)
        return (o, L.flat(S), L.flat(slots), 8192, B, N), [o]
    rowop("pmhip_remask_slots", remask_slots, [ops.remask_slots(ids.clone(), S, slots, 8192)])
    z, tok = rnd(B, N, E), rnd(E, seed=1)
    noise = t((rng.integers(0, N // 3, (B, N)) / N).astype(np.float32))

    def rmask(L):
        x, m = L.out(B * N, E, f32, flat=True), L.out(B, N, f32, flat=True)
        return (L.flat(z), L.flat(noise), L.flat(tok), 100, x, m, B, N, E), [x, m]
    rowop("pmhip_random_mask", rmask, list(ops.random_mask(z, noise, tok, 100)))


def test_rowop_vq_quantize():
    """z_out, idx_out and loss framed; the scratch is framed at exactly pmhip_vq_scratch_bytes: nothing beyond it may be written"""
    M, V, E = 300, 1000, 16
    cb, z = rnd(V, E), rnd(M, E, scale=0.3, seed=1)
    en, sq = ops.vq_prepare(cb)
    nbytes = _lib.load().pmhip_vq_scratch_bytes(M, V)

    def vq(L):
        zo, idx, loss = L.out(M, E, f32, flat=True), L.out(M, 1, i64, flat=True), L.out(1, 1, f32, flat=True)
        scratch = L.out(1, nbytes, torch.uint8, flat=True)
        return (L.flat(z), L.flat(en), L.flat(sq), 0.25, zo, idx, loss, scratch, M, V, E), [zo, idx, loss]
    z_out, idx, loss = ops.vq_quantize(z, en, sq, 0.25)
    rowop("pmhip_vq_quantize", vq, [z_out, idx, loss])
