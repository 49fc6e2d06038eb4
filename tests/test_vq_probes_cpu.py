"""The quantiser probes can fail: on the CPU, against a numpy restatement of vq.hip (vq_probes.emulate).

1. The fault-free restatement equals oracle/vq_ref.c bit for bit (idx, zn, dmin, en, sq) on every case that
   tests/test_gpu_vq_probes.py launches, and the planted expectations of `duplicates` and `identity` -- computed without the oracle --
   agree with it, at distance exactly 0.
2. The `near_tie` inputs are what they claim to be: exact ties on at least 40 % of the rows, gaps of at most 2 ulp on at least 90 %,
   at least V / 16 different answers.  These are conditions on the inputs, met by the oracle alone.
3. The same restatement with ONE fault of vq_probes.FAULTS gives other indices (or another z_out) on the family meant for it, while
   the i.i.d. family of test_vq_bit_exact_against_c_oracle lets a reversed dot chain through.
4. The geometry that the messages and the copy sets rely on restates the kernel's loops.

Measured here (rows with gap == 0 / gap <= 2 ulp / indices changed by dot_descending_k / by dot_unfused / by dist_reassociated, M = 600):
    E =  8   V = 1000  0.768 1.000 0.873 0.640 0.423      V = 2304  0.732 1.000 0.860 0.673 0.407
    E = 16   V = 1000  0.745 1.000 0.933 0.625 0.423      V = 2304  0.715 1.000 0.923 0.658 0.395
    E = 32   V = 1000  0.647 1.000 0.967 0.527 0.332      V = 2304  0.605 1.000 0.945 0.520 0.343
    E = 64   V = 1000  0.538 1.000 0.967 0.468 0.290      V = 2304  0.513 1.000 0.972 0.408 0.278
"""
import numpy as np
import pytest

import vq_probes as P
from oracle import vq_ref

_CACHE = {}


def _freeze(d):
    for x in d.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return d


def _rows(case):
    """the rows the restatement is run on.  `identity` at M = V > 2000 costs V^2 E fmaf: there, the four rows on each side of
    every tile edge and every fifth row"""
    name, _, V, _ = case
    j = np.arange(V)
    return j[(j % P.TC < 4) | (j % P.TC >= P.TC - 4) | (j % 5 == 0) | (j >= V - 4)] if name == "identity" else slice(None)


def _case(case):
    """family, oracle and fault-free restatement of one case: computed once, never modified"""
    if case not in _CACHE:
        fam = P.build(case)
        en, sq = vq_ref.prepare(fam["cb"])
        idx, zn, dmin, gap = vq_ref.quantize(fam["z"], en, sq)
        rows = _rows(case)
        _CACHE[case] = dict(fam=fam, rows=rows, ref=_freeze(dict(en=en, sq=sq, idx=idx, zn=zn, dmin=dmin, gap=gap)),
                            emu=_freeze(P.emulate(fam["z"][rows], fam["cb"])))
    return _CACHE[case]


def _rejected(case, fault):
    """share of the rows on which the faulty restatement's index differs from the oracle's"""
    c = _case(case)
    got = P.emulate(c["fam"]["z"][c["rows"]], c["fam"]["cb"], fault)["idx"]
    want = c["ref"]["idx"][c["rows"]]
    with pytest.raises(AssertionError, match="wanted"):
        P.assert_idx(got, want, case[2], c["ref"]["gap"][c["rows"]], fault)
    return float(np.mean(got != want))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the restatement is the oracle
# ---------------------------------------------------------------------------------------------------------------------------------
ALL_CASES = P.GPU_CASES + [("near_tie", 32, 1000, M) for M in P.RAGGED_M] + [("identity", E, 2049, None) for E in (8, 32)]


@pytest.mark.parametrize("case", ALL_CASES, ids=P.case_id)
def test_restatement_equals_the_c_oracle(case):
    c = _case(case)
    fam, ref, emu, rows, V = c["fam"], c["ref"], c["emu"], c["rows"], case[2]
    P.assert_bits(emu["en"], ref["en"], "en")
    P.assert_bits(emu["sq"], ref["sq"], "sq")
    P.assert_bits(emu["zn"], ref["zn"][rows], "zn")
    P.assert_idx(emu["idx"], ref["idx"][rows], V, ref["gap"][rows], "restatement vs oracle")
    P.assert_bits(emu["dmin"], ref["dmin"][rows], "dmin")
    assert ref["idx"].min() >= 0 and ref["idx"].max() < V
    if fam["expect"] is not None:
        # the oracle-free expectation: the smallest index among the bitwise copies, at distance exactly 0, everything else above
        P.assert_idx(ref["idx"], fam["expect"], V, ref["gap"], "oracle vs planted expectation")
        assert (ref["dmin"] == 0).all()
        copies = np.bincount(P.first_equal_row(fam["cb"]), minlength=V)[fam["expect"]]
        assert ((ref["gap"] == 0) == (copies > 1)).all() and (ref["gap"] >= 0).all()
        zn_src, _ = P.normalize(fam["cb"][fam["expect"]])
        P.assert_bits(ref["zn"], zn_src, "zn of a row times a power of two vs en of the row")


def test_fmaf_is_singly_rounded():
    """the float64 shortcut alone rounds twice: c + a b = 1 + 2^-23 + 2^-24 - 2^-70 lies below the midpoint of two floats, its float64
    sum on it, and the tie then goes to the even neighbour above"""
    one = np.float32
    a, b, c = one(2.0 ** -12 * (1 + 2.0 ** -23)), one(2.0 ** -12 * (1 - 2.0 ** -23)), one(1 + 2.0 ** -23)
    assert one(np.float64(a) * np.float64(b) + np.float64(c)) == one(1 + 2.0 ** -22)
    assert P.fmaf(np.array([a]), np.array([b]), np.array([c]))[0] == c
    # subnormal results: 2^-149 + 2^-150 is a tie between 2^-149 and 2^-148
    tiny = P.fmaf(np.array([2.0 ** -75], P.F), np.array([2.0 ** -75], P.F), np.array([2.0 ** -149], P.F))
    assert tiny[0] == one(2.0 ** -148)
    rng = np.random.default_rng(0)
    x, y, z = (rng.standard_normal(20000).astype(P.F) for _ in range(3))
    assert np.array_equal(P.fmaf(x, y, z), P._fmaf_odd(x, y, z))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the near-tie inputs are near ties
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in P.GPU_CASES if c[0] == "near_tie" and c[2] >= 100], ids=P.case_id)
def test_near_tie_conditions(case):
    ref, V = _case(case)["ref"], case[2]
    ties, close = P.near_tie_shares(ref["gap"])
    distinct = len(np.unique(ref["idx"]))
    print(f"{P.case_id(case)}: gap == 0 on {ties:.3f} of the rows, gap <= 2 ulp on {close:.3f}, {distinct} distinct indices")
    assert ties >= 0.40 and close >= 0.90 and distinct >= V / 16, (ties, close, distinct)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. every fault is rejected by the family meant for it
# ---------------------------------------------------------------------------------------------------------------------------------
NEAR_TIE_FAULT_CASES = [("near_tie", E, 1000, 600) for E in P.WIDTHS] + [("near_tie", E, 2304, 600) for E in (32, 64)]


@pytest.mark.parametrize("case", NEAR_TIE_FAULT_CASES, ids=P.case_id)
def test_arithmetic_order_faults_are_rejected_by_near_tie(case):
    for fault, least in (("dot_descending_k", 0.25), ("dot_unfused", 0.25), ("dist_reassociated", 0.0)):
        share = _rejected(case, fault)
        print(f"{P.case_id(case)}: {fault} changes {share:.3f} of the indices")
        assert share > 0 and share >= least, (fault, share)


def test_iid_family_lets_a_reversed_dot_chain_through():
    """why this file exists: on the inputs of test_vq_bit_exact_against_c_oracle the order of the chain does not show"""
    fam = P.iid(1024, 1000, 16)
    en, sq = vq_ref.prepare(fam["cb"])
    idx = vq_ref.quantize(fam["z"], en, sq)[0]
    assert np.array_equal(P.emulate(fam["z"], fam["cb"])["idx"], idx)
    assert np.array_equal(P.emulate(fam["z"], fam["cb"], "dot_descending_k")["idx"], idx)


TIE_FAULTS = ("last_minimum", "lane_tie_keeps_lower_lane", "lane_tie_takes_other_lane", "split_merge_keeps_later")


@pytest.mark.parametrize("E,V", [(8, 2304), (16, 2304)] + [(E, 129) for E in P.WIDTHS])
def test_tie_break_faults_are_rejected_by_duplicates(E, V):
    case = ("duplicates", E, V, None)
    c = _case(case)
    fam, n_sets = c["fam"], len(c["fam"]["sets"])
    caught = set()
    for fault in TIE_FAULTS:
        if fault == "split_merge_keeps_later" and P.vq_splits(V) == 1:
            continue                                          # nothing to merge
        got = P.emulate(fam["z"], fam["cb"], fault)["idx"]
        with pytest.raises(AssertionError, match="wanted"):
            P.assert_idx(got, fam["expect"], V, c["ref"]["gap"], fault)
        wrong = got != fam["expect"]
        kinds = {fam["sets"][i][0] for i in np.unique(np.nonzero(wrong)[0] % n_sets)}
        # a fault shows on every row of a copy set or on none, and every answer it gives is another copy
        for i, (kind, codes) in enumerate(fam["sets"]):
            assert wrong[i::n_sets].all() == (kind in kinds) == wrong[i::n_sets].any(), (fault, kind)
            assert set(got[i::n_sets].tolist()) <= set(codes), (fault, kind)
        caught |= kinds
    # no copy set is idle: each one rejects at least one of the faults
    assert caught == {kind for kind, _ in fam["sets"]}, caught


@pytest.mark.parametrize("case", [c for c in P.GPU_CASES if c[0] == "antipodal"], ids=P.case_id)
def test_zero_padding_is_rejected_by_antipodal(case):
    c = _case(case)
    assert _rejected(case, "pad_codes_are_zero") > 0
    got = P.emulate(c["fam"]["z"], c["fam"]["cb"], "pad_codes_are_zero")["idx"]
    assert (got >= case[2]).any() and ((got >= case[2]).all() or case[2] > 1)     # V = 1: distance sz = 1 against 4, on every row


@pytest.mark.parametrize("case", [("identity", 16, 2049, None), ("identity", 16, 2304, None)], ids=P.case_id)
def test_a_skipped_tile_is_rejected_by_identity(case):
    c = _case(case)
    V, rows = case[2], c["rows"]
    got = P.emulate(c["fam"]["z"][rows], c["fam"]["cb"], "split_short_by_one_tile")["idx"]
    want = c["fam"]["expect"][rows]
    with pytest.raises(AssertionError, match="wanted"):
        P.assert_idx(got, want, V, None, "split_short_by_one_tile")
    # exactly the rows whose code sits in the last tile of its split
    tiles = [-(-(v1 - v0) // P.TC) for v0, v1 in P.split_ranges(V)]
    in_last_tile = np.array([P.where(j, V)[1] == tiles[P.where(j, V)[0]] - 1 for j in want])
    assert np.array_equal(got != want, in_last_tile)


@pytest.mark.parametrize("E", P.WIDTHS)
def test_clamp_and_subnormal_faults_are_rejected_by_degenerate(E):
    case = ("degenerate", E, 300, None)
    c = _case(case)
    fam, ref, emu = c["fam"], c["ref"], c["emu"]
    want_out = ref["zn"] + (ref["en"][ref["idx"]] - ref["zn"])
    P.assert_bits(emu["z_out"], want_out, "z_out")
    assert np.isfinite(want_out).all()
    D = P.DEGENERATE_CODES
    assert ref["idx"][0] == D["zero"] and ref["idx"][3] == D["zero"]              # the zero row; the overflowing row (zn = +-0)
    row = fam["spread_rows"][0]                                                   # subnormal components reach z_out
    assert ref["idx"][row] == D["spread"] and ((want_out[row] != 0) & (np.abs(want_out[row]) < 2.0 ** -126)).any()
    for fault in ("clamp_dropped", "flush_subnormals"):
        bad = P.emulate(fam["z"], fam["cb"], fault)
        differs = (bad["idx"] != ref["idx"]) | (P.bits(bad["z_out"]) != P.bits(want_out)).any(1)
        assert differs.any(), fault
        with pytest.raises(AssertionError):
            P.assert_idx(bad["idx"], ref["idx"], 300, ref["gap"], fault)
            P.assert_bits(bad["z_out"], want_out, fault)


def test_fault_list_is_covered():
    tested = {"dot_descending_k", "dot_unfused", "dist_reassociated", "pad_codes_are_zero", "split_short_by_one_tile",
              "clamp_dropped", "flush_subnormals"} | set(TIE_FAULTS)
    assert tested == set(P.FAULTS)
    with pytest.raises(AssertionError):
        P.emulate(np.zeros((1, 8), P.F), np.ones((1, 8), P.F), "no_such_fault")


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. geometry
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,splits,per_split,last", [(2047, 1, 2048, 2047), (2048, 4, 512, 512), (2049, 4, 640, 129), (2304, 4, 640, 384),
                                                     (129, 1, 256, 129), (1, 1, 128, 1)])
def test_where_restates_the_scan_loops(V, splits, per_split, last):
    assert (P.vq_splits(V), P.cps(V), P.TC) == (splits, per_split, 128)
    ranges = P.split_ranges(V)
    assert ranges[-1][1] - ranges[-1][0] == last and all(v0 < v1 for v0, v1 in ranges)
    seen = []
    for s in range(splits):                                   # vq_scan_kernel: blockIdx.y, the tile loop, ct, l15
        v0 = s * per_split
        v1 = min(V, v0 + per_split)
        for t0 in range(v0, v1, 128):
            for ct in range(8):
                for l15 in range(16):
                    code = t0 + ct * 16 + l15
                    if code < v1:
                        assert P.where(code, V) == (s, (t0 - v0) // 128, ct, l15), code
                        seen.append(code)
    assert seen == list(range(V))


def test_row_where_restates_the_store_loop():
    rows = [(P.row_where(256 * b + 64 * w + 16 * rt + 4 * g + r), (b, w, rt, g, r))
            for b in range(3) for w in range(4) for rt in range(4) for g in range(4) for r in range(4)]
    assert all(got == want for got, want in rows)
    text = P.describe(321, 2048, 127, 2049, gap=2.0 ** -22)
    assert "row 321 (block 1, wave 1, row tile 0, g 0, r 1)" in text and "got code 2048 (split 3, tile 1, group 0, lane 0)" in text
    assert "wanted 127 (split 0, tile 0, group 7, lane 15)" in text and "1 ulp" in text
    assert "NOT a code" in P.describe(0, 17, 3, 17)


@pytest.mark.parametrize("V", [129, 2049, 2304])
def test_copy_sets_straddle_what_they_claim(V):
    sets = P.copy_sets(V)
    kinds = [k for k, _ in sets]
    codes = [j for _, cs in sets for j in cs]
    assert len(sets) % 2 == 1 and len(set(codes)) == len(codes) and max(codes) < V
    W = {k: [P.where(j, V) for j in cs] for k, cs in sets}
    same_group = lambda a, b: a[:3] == b[:3]
    a, b = W["adjacent_lanes"]
    assert same_group(a, b) and b[3] == a[3] + 1
    a, b = W["group_ends"]
    assert same_group(a, b) and (a[3], b[3]) == (0, 15)
    a, b = W["same_lane_next_group"]
    assert a[:2] == b[:2] and b[2] == a[2] + 1 and a[3] == b[3]
    a, b = W["higher_lane_earlier_group"]
    assert a[:2] == b[:2] and b[2] == a[2] + 1 and a[3] > b[3]
    a, b = W["first_last"]
    assert dict(sets)["first_last"] == (0, V - 1) and a == (0, 0, 0, 0)
    if V == 129:
        assert kinds == ["adjacent_lanes", "group_ends", "same_lane_next_group", "higher_lane_earlier_group", "first_last"]
        assert b == (0, 1, 0, 0)                              # the last code: alone in the second tile
        return
    a, b = W["same_lane_next_tile"]
    assert a[0] == b[0] and b[1] == a[1] + 1 and a[2:] == b[2:]
    a, b = W["tile_edge"]
    assert a[0] == b[0] and (a[1:], b[1:]) == ((0, 7, 15), (1, 0, 0))
    last_tile = P.cps(V) // P.TC - 1
    for s in (1, 2, 3):                                       # every split edge
        a, b = W[f"split_edge_{s}"]
        assert (a, b) == ((s - 1, last_tile, 7, 15), (s, 0, 0, 0))
        a, b = W[f"same_offset_next_split_{s}"]
        assert (a[0], b[0]) == (s - 1, s) and a[1:] == b[1:]
    a, b, c = W["three_splits"]
    assert (a[0], b[0], c[0]) == (0, 1, 2) and a[1:] == b[1:] == c[1:]
    # the finished codebook holds exactly these copies, and the planted expectation is the first of each
    fam = P.duplicates(8, V)
    first = P.first_equal_row(fam["cb"])
    assert {j: int(first[j]) for j in range(V) if first[j] != j} == {j: cs[0] for _, cs in sets for j in cs[1:]}
    assert fam["z"].shape[0] == 64 * len(sets) + 5 and np.array_equal(fam["expect"], np.array([cs[0] for _, cs in sets])[np.arange(len(fam["z"])) % len(sets)])
    for i in range(len(sets)):                                # every copy set visits every row position of a wave, and the last block
        rows = np.arange(i, len(fam["z"]), len(sets))
        assert set(rows % 64) == set(range(64)) and len(set(rows // 64)) > 4 and rows.max() >= len(fam["z"]) // 256 * 256
