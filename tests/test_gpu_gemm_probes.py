"""The GEMMs without a folded LayerNorm -- the residual-stream producers (pmhip_gemm_hilo, _stats, _center), the f32-residual
pmhip_gemm and the unfolded plain, head-split and SwiGLU calls -- ELEMENT by element, on every kernel route.

The producer tests of test_gpu_ops.py, test_gpu_abi_memory.py and test_gpu_fuzz.py hold one number per call (max |err| / max
|ref|) and absolute tolerances on unit-scale rows.  Here the `selector` family of tests/gemm_probes.py must come out bit for bit
(two ones per row of A, one in the first and one in the last K-tile, coded weights, bias, residual and centre: every f32
operation is exact, so a dropped, doubled or foreign K-tile, a residual, bias or centre from the wrong row or column, a shift
from the wrong wave or statistics in the wrong part change a NAMED element), the `hetero` family (row spreads over 2^-3 .. 2^4,
means out to 8 spreads) is held element-wise to the derived bound with no factor on top, the unfolded calls equal the folded
ones under the identity fold, and the large launches equal the small launches they are documented to equal.
tests/test_gemm_probes_cpu.py shows on the CPU that these checks reject each fault of gemm_probes.FAULTS.

Routes (dispatch() in csrc/gemm.hip for ln == NULL, restated in gemm_probes.route_of):
    128x2   128x128 two-stage                         128x4   128x128 four-stage, eight waves (at most 256 tiles, K >= 256)
    2b      256x128, two workgroups per CU (bf16 residual GEMMs, >= 192 tiles, not served by the 256x256 kernel)
    256     256x256, one tile per workgroup           256p    256x256 persistent: 256 workgroups walk the tiles
    f32     128x128 two-stage on f32 operands

The centred selector case takes the device's reciprocal of 1.0 to be 1.0 (the SwiGLU index probes of test_gpu_fold_probes.py
rest on the same fact).
"""
import numpy as np
import pytest
import torch

import fold_probes as F
import gemm_probes as P
from gpu_common import dev, n, t
from paintmind_amd import ops

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
QKV = [ops.PART_Q, ops.PART_K, ops.PART_V]

PRODUCERS = [(route, shape) for route, shapes in P.PRODUCER_SHAPES.items() for shape in shapes]
SELECTOR_VARIANTS = ("pair-modulo", "pair-center2", "pair-center1", "f32res-modulo")
HETERO_VARIANTS = ("pair", "pair-center", "f32res")
_ids = lambda cases: ["-".join(str(x) for x in (c[0],) + tuple(c[1]) + tuple(c[2:])) for c in cases]
SELECTOR_CASES = [(r, s, v) for r, s in PRODUCERS for v in SELECTOR_VARIANTS]
HETERO_CASES = [(r, s, v) for r, s in PRODUCERS for v in HETERO_VARIANTS]


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


class Dev:
    """a call's operands on the device"""

    def __init__(self, call, kind):
        dt = BF if call["dtype"] == "bf16" else F32
        self.kind, self.M = kind, call["a"].shape[0]
        self.a, self.w = t(call["a"], dt), t(call["w"], dt)
        self.bias = None if call.get("bias") is None else t(call["bias"])
        R = self.R = call["res_rows"]
        if kind == "f32res":
            self.res = t(call["res"][:R])
        elif kind == "pair":
            self.rh, self.rl = t(call["res_hi"][:R], BF), t(call["res_lo"][:R], BF)
            self.coef = None if call["center_coef"] is None else t(call["center_coef"])
            self.shift0 = None if call["shift0"] is None else t(call["shift0"])
            self.extra, self.mode, self.stats = call["center_extra"], call["shift_mode"], call["stats"]
        self.heads, self.tokens, self.q_scale = call.get("heads"), call.get("tokens"), call.get("q_scale")


def _launch(x, rows=None):
    """one launch of the kind's entry point on rows [r0, r1) of the call (the residual without a row modulo then) -> dict of tensors"""
    r0, r1 = rows or (0, x.M)
    a = x.a[r0:r1].contiguous()
    if x.kind == "plain":
        return dict(out=ops.gemm(a, x.w, x.bias, out_dtype=F32))
    if x.kind == "swiglu":
        return dict(out=ops.gemm_swiglu(a, x.w, x.bias))
    if x.kind == "heads":
        q, k, vt = ops.gemm_heads(a, x.w, x.heads, x.tokens, QKV, x.q_scale)
        return dict(q=q, k=k, vt=vt)
    mod = x.R if x.R < x.M else 0
    assert not (mod and rows)
    if x.kind == "f32res":
        return dict(out=ops.gemm(a, x.w, x.bias, residual=x.res if mod else x.res[r0:r1].contiguous(), res_rows=mod, out_dtype=F32))
    rh, rl = (x.rh, x.rl) if mod else (x.rh[r0:r1].contiguous(), x.rl[r0:r1].contiguous())
    if x.coef is None and not x.mode:
        res = ops.gemm_hilo(a, x.w, rh, rl, bias=x.bias, res_rows=mod, stats=x.stats)
        shift = None
    else:
        shift = x.shift0[r0:r1].clone()
        res = ops.gemm_hilo_center(a, x.w, rh, rl, bias=x.bias, center_coef=None if x.coef is None else x.coef[r0:r1].contiguous(), shift=shift,
                                   shift_mode=x.mode, stats=x.stats, center_extra=x.extra)
    out = dict(hi=res[0], lo=res[1])
    if x.stats:
        out["parts"] = res[2]
    if shift is not None:
        out["shift"] = shift
    return out


def _numpy(x, out):
    """what _launch returned -> the result dict of gemm_probes (heads: the flat [M, N] matrix; the padding stays zero)"""
    if x.kind == "heads":
        T = x.tokens
        assert not out["k"][:, :, T:].any() and not out["vt"][..., T:].any(), "the padding of K / V^T was written"
        return dict(out=P.heads_to_flat(n(out["q"]), n(out["k"][:, :, :T]), n(out["vt"][..., :T])))
    return {k: n(v) for k, v in out.items()}


def _selector_call(shape, variant):
    M, N, K = shape
    st, rows = N % 64 == 0, 200 if M < 1024 else 1000
    if variant == "pair-modulo":
        return "pair", P.selector_call("pair", M, N, K, res_rows=rows, stats=st)
    if variant == "pair-center2":
        return "pair", P.selector_call("pair", M, N, K, center=2, stats=st)
    if variant == "pair-center1":
        return "pair", P.selector_call("pair", M, N, K, center=1)
    return "f32res", P.selector_call("f32res", M, N, K, res_rows=rows)


@pytest.mark.parametrize("route,shape,variant", SELECTOR_CASES, ids=_ids(SELECTOR_CASES))
def test_selector_producers(route, shape, variant):
    """Producers and the f32 residual GEMM on the selector family: the hi and lo planes (or the f32 output), the shift of modes
    1 and 2 and the part sums equal the expectation bit for bit; the part squares are within stat_bounds.  The residual of the
    `modulo` variants has 200 (1000) rows, which divides neither 16 nor 128 nor the tile.  The 2b route is confirmed by its
    timing family."""
    M, N, K = shape
    assert P.route_of(M, N, K, True) == route
    kind, call = _selector_call(shape, variant)
    x = Dev(call, kind)
    got = _numpy(x, _launch(x))
    want = P.expect_selector_chunked(call, kind)
    msgs = P.check_selector(got, want, call, kind, P.walk_of(M, N, K, True), f"selector {variant} {M}x{N}x{K}")
    assert not msgs, f"{len(msgs)} failures:\n" + "\n".join(msgs)
    if variant in ("pair-modulo", "f32res-modulo"):
        assert launches("gemm_resid2b", lambda: _launch(x)) == (1 if route == "2b" else 0)


@pytest.mark.parametrize("route,shape,variant", HETERO_CASES, ids=_ids(HETERO_CASES))
def test_hetero_producers(route, shape, variant):
    """Producers and the f32 residual GEMM on heterogeneous rows: every element within the derived bound (gemm_probes.reference,
    check_hetero), the statistics of the new hi plane within stat_bounds.  Centred: center_coef is what pmhip_ln_coef computes
    for the residual hi plane, the centre of the reference is the kernel's own (shift0 = 0, mode 2, read back) and is itself
    held to its bound against float64 of center_coef.  The persistent shape is referenced on the 256-row blocks that hold a
    second tile of a walk, plus the first and the last.

    Largest err / bound measured on the MI355X, per route (value check hi + lo | centre | f32 output; the fault-free numpy
    restatement stays at or below 0.5): 128x2 0.29 | 0.24 | 0.012, 128x4 0.19 | 0.29 | 0.004, 2b 0.43 | 0.28 | 0.037,
    256 0.044 | 0.24 | 0.001, 256p 0.045 | 0.27 | 0.001; part sums and squares at most 0.009; |lo| / U |hi| reaches 1.0, as
    round-to-nearest does."""
    M, N, K = shape
    kind = "f32res" if variant == "f32res" else "pair"
    call = P.hetero_call(kind, M, N, K, center=variant == "pair-center", stats=N % 64 == 0)
    x = Dev(call, kind)
    if variant == "pair-center" and N <= 1024:         # (pmhip_ln_coef serves rows of up to 1024 columns; wider: the f32 rounding of float64 statistics)
        x.coef = ops.ln_coef(x.rh)
        call["center_coef"] = n(x.coef)
    walk = P.walk_of(M, N, K, True)
    rows = P.walked_blocks(walk) if route == "256p" else None
    ratios, msgs = P.check_hetero(_numpy(x, _launch(x)), call, kind, walk, rows, f"hetero {variant} {M}x{N}x{K}")
    print(f"gemm hetero route {route} {variant} {M}x{N}x{K}: largest err / bound", ratios)
    assert not msgs, "\n".join(msgs)


UNFOLDED_CASES = ([(P.UNFOLDED_ROUTE[r], e, s, F.TOKENS, "bf16") for (r, e), shapes in F.SHAPES.items() for s in shapes]
                  + [(r, "heads", s, 200, "bf16") for r, s in P.HEADS_T200.items()] + [("f32", "plain", P.F32_SHAPE, F.TOKENS, "f32")])


@pytest.mark.parametrize("route,epi,shape,tokens,dtype", UNFOLDED_CASES, ids=["-".join(str(x) for x in (c[0], c[1]) + c[2] + (f"t{c[3]}", c[4])) for c in UNFOLDED_CASES])
def test_selector_unfolded(route, epi, shape, tokens, dtype):
    """The unfolded plain, head-split and SwiGLU calls on the selector family, bit for bit, on the four routes they take without
    a fold, on f32 operands, and with 200 tokens per image on the two FULL routes (Q / K rows that cross an image inside a wave,
    V^T blocks that are not whole)."""
    M, N, K = shape
    assert P.route_of(M, N, K, False, dtype) == route
    call = P.selector_call(epi, M, N, K, dtype, tokens=tokens)
    x = Dev(call, epi)
    msgs = P.check_selector(_numpy(x, _launch(x)), P.expect_selector_chunked(call, epi), call, epi, P.walk_of(M, N, K, False, dtype),
                            f"selector {epi} {M}x{N}x{K} tokens {tokens} {dtype}")
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("epi", F.EPILOGUES)
def test_unfolded_equals_the_identity_fold(epi):
    """ln_apply4 under the identity fold (coef = (1, 0), c = d = 0) is fma(1, acc, fma(0, 0, 0)) = acc: the unfolded call equals
    the folded one bit for bit at every shape of fold_probes.SHAPES."""
    failures = []
    for (route, e), shapes in F.SHAPES.items():
        for M, N, K in shapes if e == epi else ():
            rng = np.random.default_rng([29, M, N, K])
            a, w = t(P.bf16_round(P.hetero_rows(M, K, 3)[0]), BF), t(P._gauss_weights(N, K, 7), BF)
            bias = None if epi == "heads" else t((0.5 + rng.standard_normal(N)).astype(np.float32))
            coef = torch.tensor([1.0, 0.0], device=dev()).repeat(M, 1).contiguous()
            c = d = torch.zeros(N, device=dev())
            if epi == "plain":
                got, want = [ops.gemm(a, w, bias, out_dtype=F32)], [ops.gemm_ln(a, w, coef, c, d, bias=bias, out_dtype=F32)]
            elif epi == "heads":
                got, want = ops.gemm_heads(a, w, F.HEADS, F.TOKENS, QKV, F.Q_SCALE), ops.gemm_heads_ln(a, w, F.HEADS, F.TOKENS, QKV, F.Q_SCALE, coef, c, d)
            else:
                got, want = [ops.gemm_swiglu(a, w, bias)], [ops.gemm_swiglu_ln(a, w, bias, coef, c, d)]
            flat = lambda o: P.heads_to_flat(*(n(v) for v in o)) if epi == "heads" else n(o[0])
            if not all(torch.equal(g, v) for g, v in zip(got, want)):
                failures.append(P.first_difference(flat(got), flat(want), epi, F.walk_of(M, N, K), f"route {route} {epi} {M}x{N}x{K}: unfolded (got) against the identity fold (want)"))
    assert not failures, "\n".join(failures)


def _equals_small_launches(M, N, K):
    """the centred producer with statistics and a running shift on the whole shape against 128x128 launches over 256-row chunks"""
    call = P.hetero_call("pair", M, N, K, center=True, stats=True, seed=1)
    call["shift0"] = P.row_code(np.arange(M), 1).astype(np.float32)
    x = Dev(call, "pair")
    big = _launch(x)
    assert P.route_of(256, N, K, True) in ("128x2", "128x4")
    small = [_launch(x, (r0, r0 + 256)) for r0 in range(0, M, 256)]
    cat = {k: torch.cat([s[k] for s in small], 0) for k in big}
    walk = P.walk_of(M, N, K, True)
    msgs = [P.first_difference(n(big[k]).reshape(M, -1), n(cat[k]).reshape(M, -1), "plain", walk, f"{k} of the {walk.route} launch {M}x{N}x{K} (got) against "
                               f"128x128 launches of 256 rows (want; parts and shift: the column is the index in the row)")
            for k in big if not torch.equal(big[k], cat[k])]
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("route", ["256", "256p"])
def test_256_producers_equal_128_launches(route):
    """'Same MFMA chain per element' (csrc/gemm.hip): planes, statistics and shift of the 256x256 and the persistent producer
    equal those of 128x128 launches over 256-row chunks, on every row."""
    for M, N, K in P.PRODUCER_SHAPES[route]:
        _equals_small_launches(M, N, K)


def test_2b_producer_equals_128_launches():
    """the same for the two-workgroups-per-CU kernel (csrc/gemm2b.hip: K-tiles in order, the two k-halves of a K-tile in order)"""
    for M, N, K in P.PRODUCER_SHAPES["2b"]:
        _equals_small_launches(M, N, K)
