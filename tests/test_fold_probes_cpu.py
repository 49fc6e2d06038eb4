"""The fold probes can fail: on the CPU, against a numpy restatement of the folded epilogue.

At every (route, epilogue, shape) of fold_probes.SHAPES -- cut down to 512 rows (and 512 columns for the plain epilogue), i.e. two
256x256 or four 128x128 tiles per dimension, where the full shape would take seconds; the route D walk then runs with half as
many workgroups as tiles (one fewer where the second tiles would all stay in their tile row), so that every workgroup walks two -- the fault-free restatement reproduces the `index` family exactly
and stays at or below HALF of the element-wise bound on the `hetero` family, and the same restatement with ONE fault of
fold_probes.FAULTS is rejected by both families: `index` differs somewhere (a row fault in at least 90 % of the rows it touches),
`hetero` exceeds the bound.  tests/test_gpu_fold_probes.py holds the kernels to exactly these checks.

The half-bound condition and the bf16 epilogues.  The bound grants a bf16 result U |ref| for its one output rounding, and
round-to-nearest ATTAINS that (a value just above a power of two): over 10^6 elements the rounded result's err / B comes out
at 0.9 .. 1 wherever the f32 part of the bound is small against U |ref|, for a correct kernel as for this restatement.  Nothing
is wrong with the derivation there and a factor on U would only blunt the probe, so for `heads` and `swiglu` the half-bound
condition is asserted where it is meaningful -- on the value IN FRONT of the output rounding, against the bound without its U
term -- and the rounded result is held to the whole bound (<= 1) like the kernels are.  The f32 epilogue is held to 0.5 as is.
"""
import numpy as np
import pytest

import fold_probes as P

CASES = [(route, epi, shape) for (route, epi), shapes in P.SHAPES.items() for shape in shapes]
CASE_IDS = [f"{r}-{e}-{m}x{n}x{k}" for r, e, (m, n, k) in CASES]
_CACHE = {}


def _freeze(d):
    for x in d.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return d


def _case(route, epi, shape):
    """the cut-down case: its walk, the index call(s) and the hetero call with reference and bound; computed once, never modified"""
    key = (route, epi, shape)
    if key not in _CACHE:
        M, N, K = shape
        Mc, Nc = min(M, 512), (min(N, 512) if epi == "plain" else N)
        tile = 128 if route in "AB" else 256
        nt = (Mc // tile) * (Nc // tile)
        walk = P.Walk(Mc, Nc, tile, P.CHUNK128 if route in "AB" else P.CHUNK256, None, route)
        for grid in range(nt // 2, 0, -1) if route == "D" else ():        # the largest grid whose second tiles change the tile row
            walk = P.Walk(Mc, Nc, tile, P.CHUNK256, grid, route)
            if (walk.previous_m() != np.arange(walk.tiles_m)[:, None]).any():
                break
        index = [_freeze(P.index_call(epi, Mc, Nc, K, v)) for v in ((0, 1) if epi == "swiglu" else (0,))]
        het = P.hetero_call(epi, Mc, Nc, K)
        het["ref"], het["B"] = P.reference(het, epi)
        _CACHE[key] = dict(walk=walk, index=index, hetero=_freeze(het))
    return _CACHE[key]


def test_helpers():
    v = P._code(np.arange(512))
    assert P.is_bf16(v) and len(np.unique(v)) == 512 and np.abs(v).min() > 1 and np.abs(v).max() == 4
    # row codes: the magnitudes differ at every distance that a row fault of the kernels can have
    r = np.arange(11008 + 256 * 64)
    for which in range(4):
        m = np.abs(P.row_code(r, which))
        assert P.is_bf16(m) and m.min() > 1
        for dist in (1, 4, 8, 16, 64, 128) + tuple(256 * k for k in range(1, 65)):
            assert (m[dist:] != m[:-dist]).all(), (which, dist)
        assert (m != np.abs(P.row_code(r ^ 128, which))).all() and (m != np.abs(P.row_code(r & ~15, which)))[r % 16 != 0].all()
    assert (np.abs(P.row_code(r, 0)) != np.abs(P.row_code(r, 2))).all() and (np.abs(P.row_code(r, 1)) != np.abs(P.row_code(r, 3))).all()
    assert (P.row_code(r, 0, signed=False) > 1).all() and (P.row_code(r, 0) < 0).any()
    n = np.arange(4096)
    for dist in (1, 4, 16, 64):
        assert (P._col_kind(n) != P._col_kind(n + dist)).mean() >= 0.7        # (not where the shift carries into the next folded bit)
        assert (P._code((37 * n + 11) % 512) != P._code((37 * (n + dist) + 11) % 512)).all()
    assert all(P._col_kind(n[i:i + 4]).sum() == 2 for i in range(0, 4096, 4))
    # layouts
    x = np.arange(512 * 1536, dtype=np.float32).reshape(512, 1536)
    q, k, vt = P.flat_to_heads(x, 8, 256)
    assert q.shape == (2, 8, 256, 64) and vt.shape == (2, 8, 64, 256) and np.array_equal(P.heads_to_flat(q, k, vt), x)
    assert q[1, 3, 5, 7] == x[256 + 5, 3 * 64 + 7] and k[1, 3, 5, 7] == x[256 + 5, 512 + 3 * 64 + 7] and vt[1, 3, 7, 5] == x[256 + 5, 1024 + 3 * 64 + 7]
    i1, i2 = P.swiglu_cols(64)
    assert i1[:18].tolist() == list(range(16)) + [32, 33] and i2[:2].tolist() == [16, 17] and sorted(np.concatenate([i1, i2]).tolist()) == list(range(128))
    assert P.gemm_col("swiglu", 17) == 33 and P.gemm_col("heads", 17) == 17
    # reporting
    call = dict(coef=np.array([[2.0, 3.0]] * 256, np.float32))
    walk = P.walk_of(256, 256, 128)
    ratio, msg = P.check_bound(np.array([[1.0, np.nan]]), np.ones((1, 2)), np.ones((1, 2)), call, "plain", walk, "x")
    assert ratio == np.inf and "(row, column) = (0, 1)" in msg and "route B" in msg and "(a_r, b_r) = (2.0, 3.0)" in msg
    assert P.worst_ratio(np.zeros((1, 2)), np.zeros((1, 2)), np.zeros((1, 2)))[0] == 0.0       # exact zeros under a zero bound pass
    assert P.first_difference(np.ones((2, 2)), np.ones((2, 2)), "plain", walk) is None
    assert "first (row, column) = (1, 0)" in P.first_difference(np.array([[1.0, 1.0], [2.0, 1.0]]), np.ones((2, 2)), "plain", walk)


def test_shapes_reach_their_routes():
    """every shape of the table takes the route it is listed under, with the tile counts the table's comment gives; the walk of
    every shape is a bijection, and in route D (and only there) some workgroup walks a second tile"""
    t256 = {}
    for (route, epi), shapes in P.SHAPES.items():
        for M, N, K in shapes:
            assert P.route_of(M, N, K) == route and M % 256 == 0 and N % 256 == 0 and K % 128 == 0, (route, epi, M, N, K)
            assert N == {"heads": 3 * P.HEADS * 64, "swiglu": 2048}.get(epi, N) and M % P.TOKENS == 0
            walk = P.walk_of(M, N, K)
            assert sorted(walk.order.ravel().tolist()) == list(range(walk.tiles_m * walk.tiles_n))
            assert (walk.step().max() == 1) == (route == "D"), (route, epi, int(walk.step().max()))
            t256[route, epi, K] = (M // 256) * (N // 256)
    assert [t256["C", "plain", 128], t256["C", "heads", 128], t256["C", "swiglu", 384]] == [132, 132, 136]
    assert [t256["D", "plain", 128], t256["D", "heads", 128], t256["D", "swiglu", 384]] == [272, 258, 264]
    assert t256["B", "plain", 256] == 72
    # the thresholds themselves, from both sides
    assert P.route_of(2048, 2048, 256) == "A" and P.route_of(2048, 2048, 128) == "B" and P.route_of(2048, 2304, 256) == "B"
    assert P.route_of(4096, 2048, 256) == "B" and P.route_of(4096, 2304, 256) == "C" and P.route_of(4096, 4096, 256) == "C" and P.route_of(4096, 4352, 256) == "D"


@pytest.mark.parametrize("route,epi,shape", CASES, ids=CASE_IDS)
def test_fault_free_emulation_reproduces_the_index_family_exactly(route, epi, shape):
    for call in _case(route, epi, shape)["index"]:
        assert not call["h"].any() and (np.abs(call["coef"][:, 0]) > 1).all()
        assert len(np.unique(call["expect"])) > 100
        out = P.emulate(call, epi)
        assert np.array_equal(out, call["expect"])
        assert np.array_equal(P.emulate(call, epi, round_out=False), call["expect"])     # exact in f32 already: rounding changes nothing


@pytest.mark.parametrize("route,epi,shape", CASES, ids=CASE_IDS)
def test_fault_free_emulation_stays_below_half_the_bound(route, epi, shape):
    case = _case(route, epi, shape)
    het, walk = case["hetero"], case["walk"]
    # the family is what it says: row spreads over 2^-3 .. 2^4, means out to several spreads, c and d changing between neighbours
    h = het["h"].astype(np.float64)
    std, off = h.std(1), np.abs(h.mean(1)) / h.std(1)
    assert std.min() < 0.2 and std.max() > 8 and off.max() > 6 and off.min() < 0.5 and P.is_bf16(het["h"]) and P.is_bf16(het["wg"])
    assert np.median(np.abs(np.diff(het["c"]))) > 0.3 and np.median(np.abs(np.diff(het["d"]))) > 0.3
    ratio, msg = P.check_bound(P.emulate(het, epi), het["ref"], het["B"], het, epi, walk, "hetero")
    assert msg is None, msg
    if epi == "plain":
        half = ratio
    else:                                            # module docstring: the value in front of the rounding, the bound without U |ref|
        half, _ = P.worst_ratio(P.emulate(het, epi, round_out=False), het["ref"], het["B"] - P.U * np.abs(het["ref"]))
    print(f"{route} {epi} {shape}: fault-free err / B = {ratio:.3f}" + ("" if epi == "plain" else f", in front of the output rounding {half:.3f}"))
    assert half <= 0.5, half


@pytest.mark.parametrize("fault", P.FAULTS)
def test_every_fault_is_rejected_by_both_families(fault):
    applied, report = 0, []
    for route, epi, shape in CASES:
        case = _case(route, epi, shape)
        walk, het = case["walk"], case["hetero"]
        if not P.fault_applies(fault, het, walk):
            continue
        applied += 1
        ratio, _ = P.worst_ratio(P.emulate(het, epi, fault, walk), het["ref"], het["B"])
        assert ratio > 1.0, f"{fault} passes the hetero bound at {route} {epi} {shape}: err / B = {ratio}"
        seen = []
        for call in case["index"]:
            bad = P.emulate(call, epi, fault, walk) != call["expect"]
            assert bad.any(), f"{fault} passes the index probe at {route} {epi} {shape}"
            seen.append(bad.any(1))
        if fault in P.ROW_FAULTS:
            touched = P.faulted_rows(fault, het, walk)
            vis = min(float(s[touched].mean()) for s in seen)
            assert touched.any() and vis >= 0.9, f"{fault} at {route} {epi} {shape}: visible in {vis:.0%} of the rows it touches"
            report.append(f"{route}-{epi}: hetero {ratio:.3g}, index rows {vis:.0%}")
        else:
            report.append(f"{route}-{epi}: hetero {ratio:.3g}, index {min(float(s.mean()) for s in seen):.0%} of rows")
    assert applied >= {"previous_tile_coef": 4, "drop_bias": 11}.get(fault, len(CASES)), applied
    print(f"{fault}: rejected by both families in all {applied} cases where it applies (hetero err / B; index rows that differ)\n  " + "\n  ".join(report))


@pytest.mark.parametrize("D", [256, 640, 1024])
def test_statistics_bounds_hold_for_an_f32_restatement_on_heterogeneous_rows(D):
    """fold_probes.stat_bounds against numpy float32 restatements of the producer's row statistics (gemm_common.h) and of their
    combination (common.h lnp_*), nparts = 4, 10 and 16: every bound holds with a factor of two to spare (they are
    worst-case sums of D roundings; rounding errors that partly cancel stay far below)."""
    hi = P.bf16_round(P.hetero_rows(512, D, seed=D)[0])
    sb = P.stat_bounds(hi)
    parts = P.parts_f32(hi)
    coef = P.coef_from_parts_f32(parts).astype(np.float64)
    r = {"part sum": np.abs(parts[..., 0] - sb["parts"][..., 0]) / sb["part_sum"], "part square": np.abs(parts[..., 1] - sb["parts"][..., 1]) / sb["part_sq"],
         "rstd": np.abs(coef[:, 0] / sb["coef"][:, 0] - 1) / sb["rstd_rel"], "b": np.abs(coef[:, 1] - sb["coef"][:, 1]) / sb["b"]}
    worst = {k: float(v.max()) for k, v in r.items()}
    print(f"D = {D} (nparts {D // 64}): largest err / bound of the f32 restatement", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 0.5 for v in worst.values()), worst
    # the restatement of the combination agrees with one made of exact parts to the same bounds (missing parts count as zero)
    c2 = P.coef_from_parts_f32(sb["parts"].astype(np.float32)).astype(np.float64)
    assert (np.abs(c2[:, 0] / sb["coef"][:, 0] - 1) <= sb["rstd_rel"]).all() and (np.abs(c2[:, 1] - sb["coef"][:, 1]) <= sb["b"]).all()
