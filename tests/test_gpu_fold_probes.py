"""The GEMMs with a folded LayerNorm against float64, ELEMENT by element, on each of the four kernel routes.

The fold tests of test_gpu_ops.py draw rows of one mean and unit spread and compare max |err| / max |ref| with 2e-2: a kernel
that normalises a row with its neighbour's coefficients passes them.  Here the `index` family of tests/fold_probes.py must come
out bit for bit (an all-zero hi plane: every output element is an exact function of ITS row's b_r and ITS column's c, d, bias),
the `hetero` family (row spreads over 2^-3 .. 2^4, means out to 8 spreads) is held element-wise to the derived bound with no
factor on top, the 256x256 launches are compared on EVERY row with the small launches they are documented to equal, and the
coefficient kernels are held to bounds relative to each row's own scale.  tests/test_fold_probes_cpu.py shows on the CPU that
these checks reject a coefficient from the wrong row, half-tile, previous tile, call or column.

Routes (dispatch() in csrc/gemm.hip, by shape alone; T256 = (M / 256) * (N / 256)):
    A  128x128 four-stage, T256 <= 64 and K >= 256 (deep128)         B  128x128 two-stage, T256 <= 128 otherwise (fold_small)
    C  256x256, one tile per workgroup, T256 <= 256 (launch256)      D  256x256 persistent: 256 workgroups walk the tiles
"""
import numpy as np
import pytest
import torch

import fold_probes as P
from gpu_common import dev, n, t
from paintmind_amd import ops

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
KINDS = [ops.PART_Q, ops.PART_K, ops.PART_V]

# (route, epilogue) -> [(M, N, K)]: the smallest shapes that reach each route.  The table lives in tests/fold_probes.py, next to the
# thresholds it follows -- deep128() (64 tiles of 256x256, K >= 256) and fold_small() (128) in csrc/gemm.hip, launch256()'s persistent
# grid (256) in csrc/gemm256.hip -- so that the CPU tests run the same shapes; a change of a threshold needs a change there.
SHAPES = P.SHAPES
ROUTE_EPI = pytest.mark.parametrize("route,epi", list(SHAPES), ids=[f"{r}-{e}" for r, e in SHAPES])


class Dev:
    """a call's operands on the device"""

    def __init__(self, call):
        self.h, self.wg = t(call["h"], BF), t(call["wg"], BF)
        self.coef, self.c, self.d = t(call["coef"]), t(call["c"]), t(call["d"])
        self.bias = None if call.get("bias") is None else t(call["bias"])
        self.heads, self.tokens, self.q_scale = call["heads"], call["tokens"], call["q_scale"]


def _launch(epi, x, rows=None, coef=None, parts=None):
    """one launch of the epilogue's entry point on rows [r0, r1) of the call -> torch tensor(s)"""
    r0, r1 = rows or (0, x.h.shape[0])
    h = x.h[r0:r1].contiguous()
    coef = (x.coef if coef is None else coef)[r0:r1].contiguous()
    if epi == "plain":
        return ops.gemm_ln(h, x.wg, coef, x.c, x.d, bias=x.bias, out_dtype=F32, parts=parts)
    if epi == "heads":
        return ops.gemm_heads_ln(h, x.wg, x.heads, x.tokens, KINDS, x.q_scale, coef, x.c, x.d, parts=parts)
    return ops.gemm_swiglu_ln(h, x.wg, x.bias, coef, x.c, x.d, parts=parts)


def _flat(epi, out):
    """what _launch returned -> the numpy [M, N] (SwiGLU: [M, Hp]) matrix of fold_probes"""
    return P.heads_to_flat(*(n(o) for o in out)) if epi == "heads" else n(out)


@ROUTE_EPI
def test_fold_index_probe(route, epi):
    """All-zero hi plane, synthetic coefficients: the whole output equals the expectation bit for bit (SwiGLU: once with the codes
    in x2 and once in x1).  At the first shape of each route the plain call also runs through pmhip_gemm_softmax_stats: the same
    logits bit for bit, and the block statistics that the stored logits give (guidance_combine with cond = uncond)."""
    failures = []
    for i, (M, N, K) in enumerate(SHAPES[route, epi]):
        assert P.route_of(M, N, K) == route
        walk = P.walk_of(M, N, K)
        for variant in ((0, 1) if epi == "swiglu" else (0,)):
            call = P.index_call(epi, M, N, K, variant, P.HEADS, P.TOKENS, P.Q_SCALE)
            x = Dev(call)
            out = _launch(epi, x)
            msg = P.first_difference(_flat(epi, out), call["expect"], epi, walk, f"index {epi} {M}x{N}x{K} variant {variant}")
            if msg:
                failures.append(msg)
            if epi == "plain" and i == 0:
                logits, stats = ops.gemm_softmax_stats(x.h, x.wg, bias=x.bias, fold=(x.coef, x.c, x.d))
                if not torch.equal(logits, out):
                    failures.append(P.first_difference(n(logits), n(out), epi, walk, f"gemm_softmax_stats logits vs gemm_ln {M}x{N}x{K}"))
                _, want = ops.guidance_combine(logits, logits, 1.0, with_stats=True)
                if not torch.equal(stats, want):
                    r, b, _ = (int(v) for v in torch.nonzero(stats != want)[0])
                    failures.append(f"gemm_softmax_stats {M}x{N}x{K}: block statistics differ from those of the stored logits, first (row, block) = "
                                    f"({r}, {b}); {walk.describe(r, b * 64)}")
    assert not failures, f"{len(failures)} failures:\n" + "\n".join(failures)


@ROUTE_EPI
def test_fold_hetero_bound(route, epi):
    """Heterogeneous rows with the coefficients pmhip_ln_coef computes for them (read back: the reference uses the device's f32
    values, so a coefficient error cannot hide an epilogue error or be hidden by one): |out - ref| <= B for every element."""
    failures, worst = [], []
    for M, N, K in SHAPES[route, epi]:
        assert P.route_of(M, N, K) == route
        call = P.hetero_call(epi, M, N, K, 0, P.HEADS, P.TOKENS, P.Q_SCALE)
        x = Dev(call)
        x.coef = ops.ln_coef(x.h)
        call["coef"] = n(x.coef)
        out = _flat(epi, _launch(epi, x))
        ref, B = P.reference(call, epi)
        ratio, msg = P.check_bound(out, ref, B, call, epi, P.walk_of(M, N, K), f"hetero {epi} {M}x{N}x{K}")
        worst.append(round(ratio, 3))
        if msg:
            failures.append(msg)
    print(f"fold hetero route {route} {epi} {SHAPES[route, epi]}: largest err / B", worst)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("epi", P.EPILOGUES)
def test_fold_routes_agree_on_every_row(epi):
    """'Bit-identical either way' on ALL rows: the route C and route D launches equal the concatenation of small launches over
    their rows -- chunks of 256 rows (route B), of 512 where K >= 256 (route A; a last chunk of 256 where M is an odd multiple);
    for the head split a chunk is a whole number of 256-token images."""
    failures = []
    for route in "CD":
        for M, N, K in SHAPES[route, epi]:
            call = P.hetero_call(epi, M, N, K, 1, P.HEADS, P.TOKENS, P.Q_SCALE)
            x = Dev(call)
            x.coef = ops.ln_coef(x.h)
            big = _launch(epi, x)
            step = 512 if K >= 256 else 256
            chunks = [(r0, min(r0 + step, M)) for r0 in range(0, M, step)]
            assert {P.route_of(r1 - r0, N, K) for r0, r1 in chunks} == {"A" if K >= 256 else "B"} and step % x.tokens == 0
            small = [_launch(epi, x, rows) for rows in chunks]
            cat = [torch.cat(parts, 0) for parts in zip(*small)] if epi == "heads" else torch.cat(small, 0)
            same = all(torch.equal(a, b) for a, b in zip(big, cat)) if epi == "heads" else torch.equal(big, cat)
            if not same:
                failures.append(P.first_difference(_flat(epi, big), _flat(epi, cat), epi, P.walk_of(M, N, K), f"route {route} {epi} {M}x{N}x{K} (got) against "
                                                   f"launches of {step} rows (want)"))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("D", [256, 640, 1024])
def test_fold_coefficients_on_heterogeneous_rows(D):
    """The producer's row statistics (pmhip_gemm_hilo_stats) and their combination (pmhip_ln_coef_parts, and the prologue of the
    four-stage 128x128 consumer) at nparts = 4, 10 and 16 -- below 8 every second half of ln_coef_row's pairs is missing, between
    8 and 16 some are -- on a stream whose rows differ in scale by 2^7: against float64 statistics of the NEW hi plane, with the
    bounds of fold_probes.stat_bounds, relative to each row's own scale."""
    M, N = 2816, 3072                                        # the route C shape; its first 512 rows and columns run route A
    assert P.route_of(M, N, D) == "C" and P.route_of(512, 512, D) == "A"
    x, _, std = P.hetero_rows(M, D, seed=D)
    rng = np.random.default_rng([19, D])
    a = P.bf16_round((0.25 * std[:, None] * rng.standard_normal((M, 64))).astype(np.float32))
    w, b0 = P._gauss_weights(D, 64, 3), (0.02 * rng.standard_normal(D)).astype(np.float32)
    rh, rl = ops.split_hilo(t(x))
    hi, lo, parts = ops.gemm_hilo(t(a, BF), t(w, BF), rh, rl, bias=t(b0), stats=True)
    h = n(hi)
    # the new plane keeps the heterogeneity
    s, off = h.astype(np.float64).std(1), np.abs(h.astype(np.float64).mean(1)) / h.astype(np.float64).std(1)
    assert s.min() < 0.2 and s.max() > 8 and off.max() > 6 and off.min() < 0.5, (s.min(), s.max(), off.min(), off.max())
    sb = P.stat_bounds(h)
    p = n(parts).astype(np.float64)
    assert p.shape == (M, D // 64, 2) and np.isfinite(p).all()
    r_sum, r_sq = np.abs(p[..., 0] - sb["parts"][..., 0]) / sb["part_sum"], np.abs(p[..., 1] - sb["parts"][..., 1]) / sb["part_sq"]
    coefp = ops.ln_coef_parts(parts)
    cp, cl = n(coefp).astype(np.float64), n(ops.ln_coef(hi)).astype(np.float64)
    r_rstd, r_b = np.abs(cp[:, 0] / sb["coef"][:, 0] - 1) / sb["rstd_rel"], np.abs(cp[:, 1] - sb["coef"][:, 1]) / sb["b"]
    x_rstd, x_b = np.abs(cp[:, 0] / cl[:, 0] - 1) / sb["rstd_rel"], np.abs(cp[:, 1] - cl[:, 1]) / sb["b"]
    print(f"D = {D} (nparts {D // 64}): largest err / bound: part sum {r_sum.max():.3f}, part square {r_sq.max():.3f}, rstd {r_rstd.max():.3f}, "
          f"b {r_b.max():.3f}; ln_coef_parts against ln_coef: rstd {x_rstd.max():.3f}, b {x_b.max():.3f} (of a doubled bound: <= 2)")
    for name, r in (("part sum", r_sum), ("part square", r_sq), ("rstd", r_rstd), ("b", r_b)):
        assert r.max() <= 1.0, f"{name}: err / bound = {r.max()} at {np.unravel_index(int(np.argmax(r)), r.shape)}"
    assert x_rstd.max() <= 2.0 and x_b.max() <= 2.0, (x_rstd.max(), x_b.max())
    # the consumers: coefficients from the parts, written to a NaN-filled coef
    wg = t(P._gauss_weights(N, D, 4), BF)
    c, d, bias = t(n(wg).astype(np.float64).sum(1).astype(np.float32)), t(rng.standard_normal(N).astype(np.float32)), t(rng.standard_normal(N).astype(np.float32))
    nan = lambda rows: torch.full((rows, 2), float("nan"), device=dev())
    for rows, cols, route in ((512, 512, "A: coefficients in the GEMM's own prologue"), (M, N, "C: pmhip_ln_coef_parts launched by the call")):
        hs, ps, ws = hi[:rows].contiguous(), parts[:rows].contiguous(), wg[:cols].contiguous()
        got_coef = nan(rows)
        got = ops.gemm_ln(hs, ws, got_coef, c[:cols].contiguous(), d[:cols].contiguous(), bias=bias[:cols].contiguous(), out_dtype=F32, parts=ps)
        want = ops.gemm_ln(hs, ws, coefp[:rows].contiguous(), c[:cols].contiguous(), d[:cols].contiguous(), bias=bias[:cols].contiguous(), out_dtype=F32)
        bad = torch.nonzero((got_coef != coefp[:rows]).any(1))
        assert len(bad) == 0, f"route {route}: the coefficients of {len(bad)} rows are not pmhip_ln_coef_parts' bit for bit, first row {int(bad[0])}"
        assert torch.isfinite(got).all() and torch.equal(got, want), f"route {route}: " + str(
            P.first_difference(n(got), n(want), "plain", P.walk_of(rows, cols, D), "parts= (got) against the coefficients passed in (want)"))
