"""The GEMM probes can fail: on the CPU, against a numpy restatement of the producer, f32-residual and unfolded epilogues.

The `selector` family is EXACT: expect_selector asserts, in float64, that every intermediate of the epilogue is a float32 value
-- here at every shape of gemm_probes.PRODUCER_SHAPES at full size for the centred producer with statistics (the variant with
the most intermediates and the largest magnitudes), and at every variant on shapes cut down to 512 rows and columns, where the
fault-free restatement must also reproduce the expectation bit for bit.  On the same cut-down shapes the fault-free restatement
stays at or below HALF of the element-wise bound of the `hetero` family, and the restatement with ONE fault of
gemm_probes.FAULTS fails the check of every family the fault names.  tests/test_gpu_gemm_probes.py holds the kernels to exactly
these checks (check_selector, check_hetero).

|lo| <= U |hi| and the statistics bounds are attained by correct roundings (round to nearest reaches half an ulp), so the
half-bound condition is asserted on the value checks (out, hi + lo, shift) and the others are held to <= 1 like the kernels are.
"""
import numpy as np
import pytest

import fold_probes as F
import gemm_probes as P

PRODUCERS = [(route, shape) for route, shapes in P.PRODUCER_SHAPES.items() for shape in shapes]
PRODUCER_IDS = [f"{r}-{m}x{n}x{k}" for r, (m, n, k) in PRODUCERS]
UNFOLDED = [(route, epi, shapes[0]) for (route, epi), shapes in F.SHAPES.items()]
_CACHE = {}


def _cut(route, shape, heads_like=False):
    """the cut-down shape and its walk; the persistent walk runs with at most half as many workgroups as tiles, so that every
    workgroup walks two (the largest such grid whose second tiles change the tile)"""
    M, N, K = shape
    Mc, Nc = min(M, 512), (N if heads_like else min(N, 512))
    if route == "2b":
        return (Mc, Nc, K), P.Walk2b(Mc, Nc)
    if route in ("256", "256p"):
        walk = P.Walk(Mc, Nc, 256, P.CHUNK256, None, route)
        for grid in range(walk.tiles_m * walk.tiles_n // 2, 0, -1) if route == "256p" else ():
            walk = P.Walk(Mc, Nc, 256, P.CHUNK256, grid, route)
            pm, pn = P.previous_tile(walk)
            if (pm != np.arange(walk.tiles_m)[:, None]).any() and (pn != np.arange(walk.tiles_n)[None, :]).any():
                break
        return (Mc, Nc, K), walk
    return (Mc, Nc, K), P.Walk(Mc, Nc, 128, P.CHUNK128, None, route)


def _producer_case(route, shape):
    """the cut-down producer case: (name, kind, selector call, hetero call) per variant, computed once"""
    key = (route, shape)
    if key not in _CACHE:
        (M, N, K), walk = _cut(route, shape)
        st = N % 64 == 0
        variants = [
            ("pair, row modulo", "pair", P.selector_call("pair", M, N, K, res_rows=200, stats=st), P.hetero_call("pair", M, N, K, stats=st, res_rows=200)),
            ("pair, centred, shift += c", "pair", P.selector_call("pair", M, N, K, center=2, stats=st), P.hetero_call("pair", M, N, K, center=True, stats=st)),
            ("pair, centred, shift <- 0", "pair", P.selector_call("pair", M, N, K, center=1), None),
            ("f32 residual, row modulo", "f32res", P.selector_call("f32res", M, N, K, res_rows=200), P.hetero_call("f32res", M, N, K, res_rows=200)),
        ]
        _CACHE[key] = (walk, variants)
    return _CACHE[key]


def _unfolded_case(route, epi, shape):
    key = (route, epi, shape)
    if key not in _CACHE:
        (M, N, K), walk = _cut(P.UNFOLDED_ROUTE[route], shape, heads_like=epi != "plain")
        _CACHE[key] = (walk, P.selector_call(epi, M, N, K))
    return _CACHE[key]


def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k][..., 0] if k == "parts" else a[k], b[k]) for k in a)


def test_shapes_reach_their_routes():
    """every shape of the tables takes the route it is listed under, from both sides of each threshold"""
    for route, shapes in P.PRODUCER_SHAPES.items():
        for M, N, K in shapes:
            assert P.route_of(M, N, K, True) == route, (route, M, N, K)
            walk = P.walk_of(M, N, K, True)
            assert sorted(walk.order.ravel().tolist()) == list(range(walk.tiles_m * walk.tiles_n))
            assert (walk.step().max() == 1) == (route == "256p")
    assert P.route_of(*P.F32_SHAPE, True, "f32") == "f32" and P.route_of(*P.F32_SHAPE, False, "f32") == "f32"
    # the table's comments: 272 tiles of 128x128 and M no multiple of 256; exactly 192 tiles of 256x128; 96 and 260 tiles of 256x256
    assert 17 * 16 == 272 and 2176 % 256 == 128 and 24 * 8 == 192 and 64 * 3 == 192 and 24 * 4 == 96 and 65 * 4 == 260
    walk = P.walk_of(16640, 1024, 1024, True)
    assert int((walk.step() >= 1).sum()) == 4 and walk.grid == 256 and len(P.walked_blocks(walk)) % 256 == 0
    # the unfolded calls of fold_probes.SHAPES: four-stage, two-stage, 256x256 and persistent without a fold
    for (route, epi), shapes in F.SHAPES.items():
        for M, N, K in shapes:
            assert P.route_of(M, N, K, False) == P.UNFOLDED_ROUTE[route], (route, epi, M, N, K)
    for route, (M, N, K) in P.HEADS_T200.items():
        assert P.route_of(M, N, K, False) == route and M % 200 == 0 and N == 3 * P.HEADS * 64
    # the thresholds, from both sides
    assert P.route_of(6144, 1024, 64, False) == "128x2" and P.route_of(5888, 1024, 64, True) == "128x2"      # 2b: a residual, 192 tiles
    assert P.route_of(6144, 1024, 960, True) == "2b" and P.route_of(6144, 1024, 1024, True) == "256" and P.route_of(6144, 1024, 128, False) == "256"
    assert P.route_of(5888, 1024, 1024, True) == "128x2" and P.route_of(16384, 1024, 1024, True) == "256" and P.route_of(16640, 1024, 1024, True) == "256p"
    assert P.route_of(2048, 2048, 256, True) == "128x4" and P.route_of(2048, 2048, 192, True) == "128x2" and P.route_of(2176, 2048, 256, True) == "128x2"
    assert P.route_of(6144, 1152, 64, True) == "2b" and P.route_of(6144, 1088, 64, True) == "128x2"           # N % 128


def test_helpers():
    # the selector columns: k1 in the first half of the first K-tile, k2 in the second half of the last one; W identifies (n, k)
    r = np.arange(16640)
    for K, ks in ((64, 64), (192, 64), (1024, 64), (128, 32)):
        k1, k2 = P.selector_k(r, K, ks)
        assert k1.min() == 0 and k1.max() == ks // 2 - 1 and k2.min() == K - ks // 2 and k2.max() == K - 1
        assert (k1[256:] != k1[:-256]).mean() > 0.9 and (k1[1:] != k1[:-1]).all()
    call = P.selector_call("pair", 256, 256, 192)
    assert F.is_bf16(call["w"]) and (call["a"].sum(1) == 2).all() and np.abs(call["w"]).min() > 1 and np.abs(call["w"]).max() <= 4
    assert all(len(np.unique(call["w"][n])) == 192 for n in (0, 100, 255))
    res = call["res_hi"].astype(np.float64) + call["res_lo"]
    assert np.abs(res).max() < 64 and np.array_equal(res * 1024, np.round(res * 1024)) and len(np.unique(res)) > 30000
    for dist in (1, 4, 8, 64):
        assert (call["bias"] != np.roll(call["bias"], -dist)).all()
    assert (res[1:] != res[:-1]).mean() > 0.99 and (res[16:] != res[:-16]).mean() > 0.99 and (res != res[np.arange(256) ^ 128]).mean() > 0.99
    assert (call["res_lo"] != call["res_lo"][:, np.arange(256) ^ 1]).mean() > 0.9
    # reporting: the wrong element, its tile and its place in the walk
    walk = P.walk_of(16640, 1024, 1024, True)
    want = dict(hi=np.ones((16640, 4), np.float32), lo=np.zeros((16640, 4), np.float32), shift=np.zeros(16640, np.float32))
    got = {k: v.copy() for k, v in want.items()}
    assert P.check_selector(got, want, None, "pair", walk) == []
    r1 = int(np.argwhere(walk.step() == 1)[0][0]) * 256 + 3
    got["hi"][r1, 2], got["shift"][r1] = 2.0, 1.0
    msgs = P.check_selector(got, want, None, "pair", walk, "x")
    assert len(msgs) == 2 and f"first (row, column) = ({r1}, 2)" in msgs[0] and "route 256p" in msgs[0] and f"first row {r1}" in msgs[1]
    assert "route 2b, 256x128 tile (m, n) = (1, 3)" in P.Walk2b(6144, 1024).describe(300, 400)


@pytest.mark.parametrize("route,shape", PRODUCERS, ids=PRODUCER_IDS)
def test_selector_is_exact_at_full_size(route, shape):
    """expect_selector's assertions (every intermediate a float32 value, magnitudes below 109, part sums integers below 2^24 on
    the 2^-10 grain) on the whole shape, for the centred producer with statistics where N allows them"""
    M, N, K = shape
    call = P.selector_call("pair", M, N, K, center=2, stats=N % 64 == 0)
    want = P.expect_selector_chunked(call, "pair")
    assert want["hi"].shape == (M, N) and F.is_bf16(want["hi"]) and F.is_bf16(want["lo"]) and len(np.unique(want["hi"])) > 1000
    assert np.array_equal(want["shift"].astype(np.float64), call["shift0"].astype(np.float64) + 0.25 - call["center_coef"][:, 1].astype(np.float64))


@pytest.mark.parametrize("route,shape", PRODUCERS, ids=PRODUCER_IDS)
def test_fault_free_emulation_reproduces_the_selector_family_exactly(route, shape):
    walk, variants = _producer_case(route, shape)
    for name, kind, sel, _ in variants:
        want = P.expect_selector(sel, kind)
        got = P.emulate(sel, kind)
        assert _same(got, want), name
        assert P.check_selector(got, want, sel, kind, walk, name) == []


@pytest.mark.parametrize("route,epi,shape", UNFOLDED + [("f32", "plain", P.F32_SHAPE)], ids=lambda v: str(v).replace(" ", ""))
def test_fault_free_emulation_reproduces_the_unfolded_selector_calls_exactly(route, epi, shape):
    if route == "f32":
        M, N, K = shape
        walk = P.walk_of(M, N, K, False, "f32")
        cases = [(kind, P.selector_call(kind, M, N, K, "f32", res_rows=200 if kind == "f32res" else 0)) for kind in ("plain", "f32res")]
        assert cases[0][1]["kstep"] == 32 and cases[0][1]["k1"].max() == 15 and cases[0][1]["k2"].min() == K - 16
    else:
        walk, call = _unfolded_case(route, epi, shape)
        cases = [(epi, call)]
    for kind, call in cases:
        want = P.expect_selector(call, kind)
        assert len(np.unique(want["out"])) > 100 and (kind in ("plain", "f32res") or F.is_bf16(want["out"]))
        got = P.emulate(call, kind)
        assert _same(got, want) and P.check_selector(got, want, call, kind, walk) == []


@pytest.mark.parametrize("route,shape", PRODUCERS, ids=PRODUCER_IDS)
def test_fault_free_emulation_stays_below_half_the_bound(route, shape):
    walk, variants = _producer_case(route, shape)
    for name, kind, _, het in variants:
        if het is None:
            continue
        # the family is what it says: row spreads over 2^-3 .. 2^4, means out to several spreads
        res = (het["res"] if kind == "f32res" else het["res_hi"]).astype(np.float64)
        std, off = res.std(1), np.abs(res.mean(1)) / res.std(1)
        assert std.min() < 0.2 and std.max() > 8 and off.max() > 6 and off.min() < 0.5
        ratios, msgs = P.check_hetero(P.emulate(het, kind), het, kind, walk, None, name)
        print(f"{route} {shape} cut to {het['a'].shape[0]}x{het['w'].shape[0]}, {name}: fault-free err / bound", ratios)
        assert msgs == [], msgs
        assert all(ratios[k] <= 0.5 for k in ("out", "hi + lo", "shift") if k in ratios), ratios


@pytest.mark.parametrize("fault", list(P.FAULTS))
def test_every_fault_is_rejected_by_the_families_it_names(fault):
    kinds, families = P.FAULTS[fault]
    applied, report = {f: 0 for f in families}, []
    for route, shape in PRODUCERS:
        walk, variants = _producer_case(route, shape)
        for name, kind, sel, het in variants:
            if "selector" in families and P.fault_applies(fault, sel, kind, walk):
                msgs = P.check_selector(P.emulate(sel, kind, fault, walk), P.expect_selector(sel, kind), sel, kind, walk, name)
                assert msgs, f"{fault} passes the selector check at {route} {shape}, {name}"
                applied["selector"] += 1
            if "hetero" in families and het is not None and P.fault_applies(fault, het, kind, walk):
                ratios, msgs = P.check_hetero(P.emulate(het, kind, fault, walk), het, kind, walk, None, name)
                assert msgs, f"{fault} passes the hetero check at {route} {shape}, {name}: {ratios}"
                applied["hetero"] += 1
                report.append(f"{route}-{shape[0]}x{shape[1]}x{shape[2]} {name}: {max(ratios.values()):.3g}")
    for route, epi, shape in UNFOLDED:
        walk, call = _unfolded_case(route, epi, shape)
        if "selector" in families and P.fault_applies(fault, call, epi, walk):
            msgs = P.check_selector(P.emulate(call, epi, fault, walk), P.expect_selector(call, epi), call, epi, walk, f"{route} {epi}")
            assert msgs, f"{fault} passes the selector check at the unfolded {route} {epi} {shape}"
            applied["selector"] += 1
    assert all(v >= 1 for v in applied.values()), applied
    print(f"{fault}: rejected in every case where it applies {applied}; hetero err / bound:\n  " + "\n  ".join(report))
