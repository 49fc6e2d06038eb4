"""The probes of the wave-per-16-query attention kernels and of the text towers' row operators can fail: on the CPU, against numpy
restatements of the kernels' arithmetic (tests/wave16_probes.py).

The fault-free restatement meets the derived bounds of tests/t5_ref.py and tests/clip_ref.py in every family at every L of the edge
list, both L_pad, every kv_lens triple and both dtypes, and the exact rows of the selector bit for bit.  The same restatement with ONE
named fault is rejected (|error| / bound > 1, or a bit of an exact row) by the family DESIGNATED for it at every (dtype, L) where the
fault can change anything (`fault_applies`, a rule about the kernel's structure that holds at three or more L per dtype).
tests/test_gpu_wave16_probes.py holds the kernels to exactly these cases and checks.

Which families see what (all L, both dtypes; the designation makes every family necessary, none is the only one to see a fault):
every family rejects the stride, padding, mask, bias-index, kv_lens, tail and diagonal faults wherever they apply.  next_query_row is
seen by the selector and gauss only (the ordered scores do not depend on the query row).  o_not_rescaled / l_not_rescaled are seen
by ordered rising, spike_last, spike_in_last_partial_block and huge_jumps everywhere, not by falling (relbias), spike_first and
very_negative, whose maximum never rises after the first block.  drop_last_key in the causal kernel touches one row per tile: ordered
and gauss see it everywhere, the selector at 14 of 24 (dtype, L).

The two precision faults are not in the list.  Worst |error| / bound with the fault (bf16; fault-free in brackets): causal p_truncated
0.86 (0.62), causal diag_p_rounded_to_bf16 0.79 (0.62): invisible.  relbias p_truncated: at most 0.98 in the selector and ordered
families, but 1.09 in gauss at L = 16, 31, 48, 64, 77 (fault-free 0.74): a truncated P may cost a whole ulp of bf16, 2 ub A against the
ub A the bound grants, so the gauss family sees it at 5 of the 12 L and not at the other 7.  Nothing was tightened or loosened for it.
"""
import numpy as np
import pytest

import clip_ref as RC
import t5_ref as RT
import wave16_probes as W

KINDS = ("relbias", "causal")
DT = {False: "f32", True: "bf16"}


def _lens_list(kind, L):
    return W.lens_sets(L) if kind == "relbias" else [None]


def _rejected(c, bf16, L_pad, lens, fault):
    r = W.reference(c, lens)
    out = W.emulate(c, bf16, L_pad, lens, fault)
    return W.worst_ratio(out, *r[DT[bf16]]) > 1.0 or W.exact_mismatch(out, r) > 0


def test_builders_are_what_they_say():
    for L in W.LS:
        sets = W.lens_sets(L)
        flat = {v for s in sets for v in s}
        assert {0, L + 5, L, 1} <= flat and {min(x, L) for x in (15, 16, 17, 31, 32, 33)} <= flat and (L == 1 or L - 1 in flat)
        assert all(len(s) == W.NB for s in sets) and W.pads(L)[0] - L < 4 and W.pads(L)[1] == W.pads(L)[0] + 12
    for kind in KINDS:
        for L in W.LS:
            for fam in W.FAMILIES[kind]:
                c = W.case(kind, fam, L)
                assert c["q"].shape == (W.NB, W.NH, L, 64) and all(W.is_bf16(c[x]) for x in "qkv")
            sel = W.case(kind, W.FAMILIES[kind][0], L)
            assert np.array_equal(sel["v"], np.round(sel["v"])) and sel["v"].min() >= 1 and sel["v"].max() <= 256    # exact in bf16
            assert not np.array_equal(sel["v"][0, 0], sel["v"][1, 0]) and not np.array_equal(sel["v"][0, 0], sel["v"][0, 1])
            rows = sum(int(W.reference(W.case(kind, fam, L), lens)["rows"].sum())
                       for fam in W.FAMILIES[kind] if fam.startswith("selector") for lens in _lens_list(kind, L))
            assert rows >= L, (kind, L, rows)                                 # the exact comparison is not empty at any L
    # the ordered patterns along the key walk: the block maxima of both block sizes
    for KB in (16, 32):
        blocks = lambda s: [s[i:i + KB].max() for i in range(0, len(s), KB)]  # noqa: E731
        up, down = blocks(W.pattern("rising", 77)), blocks(W.pattern("falling", 77))
        assert all(b > a for a, b in zip(up, up[1:])) and all(b < a for a, b in zip(down, down[1:]))
        jumps = blocks(W.pattern("huge_jumps", 77))
        assert all(b - a >= 60 for a, b in zip(jumps, jumps[1:]))
        for N in (17, 33, 49, 77):
            s = W.pattern("spike_in_last_partial_block", N)
            assert s.argmax() >= KB * ((N - 1) // KB) and s.max() - np.sort(s)[-2] >= 30
    s = W.pattern("very_negative", 77)
    assert s.max() < -1e4 and 1 <= s.max() - s.min() <= 4
    assert W.pattern("spike_first", 77).argmax() == 0 and W.pattern("spike_last", 77).argmax() == 76


@pytest.mark.parametrize("kind", KINDS)
def test_fault_rules_leave_three_lengths_per_dtype(kind):
    for fault in W.FAULTS[kind] + W.PRECISION_FAULTS[kind]:
        assert fault in W.DESIGNATED or fault in W.PRECISION_FAULTS[kind]
        counts = {bf16: sum(W.fault_applies(fault, kind, bf16, L, W.pads(L)[1]) for L in W.LS) for bf16 in (False, True)}
        assert max(counts.values()) >= 3 and all(n == 0 or n >= 3 for n in counts.values()), (fault, counts)
        if counts[False] == 0:                                               # a fault that concerns one dtype says so by rule
            assert fault in ("second_tile_dropped", "p_chunk_order", "diagonal_from_wrong_tile", "matrix_part_sees_diagonal", "p_truncated",
                             "diag_p_rounded_to_bf16") or (kind == "causal" and fault == "v_pad_not_zeroed"), fault


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_fault_free_emulation_meets_the_bound(kind, bf16):
    worst = {}
    for L in W.LS:
        for fam in W.FAMILIES[kind]:
            c = W.case(kind, fam, L)
            for lens in _lens_list(kind, L):
                r = W.reference(c, lens)
                for L_pad in W.pads(L):
                    out = W.emulate(c, bf16, L_pad, lens)
                    ratio = W.worst_ratio(out, *r[DT[bf16]])
                    assert ratio <= 1.0, (kind, fam, L, L_pad, lens, ratio)
                    assert W.exact_mismatch(out, r) == 0, (kind, fam, L, L_pad, lens)
                    group = fam.split("_")[0]
                    worst[group] = max(worst.get(group, 0.0), ratio)
                    if L_pad == W.pads(L)[1] and lens in (None, W.lens_sets(L)[0]):                       # the padding reaches nothing
                        assert np.array_equal(W.emulate(c, bf16, L_pad, lens, pad=0.0), out)
    print(f"largest |error| / bound of the fault-free {kind} emulation, {DT[bf16]}:", {k: round(v, 3) for k, v in worst.items()})
    assert worst["gauss"] > (0.2 if bf16 else 0.0)                           # the bf16 bound is not slack by an order of magnitude


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind, fault", [(k, f) for k in KINDS for f in W.FAULTS[k]])
def test_every_fault_is_rejected_by_its_family_wherever_it_applies(kind, fault, bf16):
    fams = [f for f in W.FAMILIES[kind] if f.startswith(W.DESIGNATED[fault])]
    assert fams
    applied = 0
    for L in W.LS:
        for L_pad in W.pads(L):
            if not W.fault_applies(fault, kind, bf16, L, L_pad):
                continue
            applied += 1
            assert any(_rejected(W.case(kind, fam, L), bf16, L_pad, lens, fault) for fam in fams for lens in _lens_list(kind, L)), \
                (kind, fault, DT[bf16], L, L_pad)
    assert applied >= 3 or not any(W.fault_applies(fault, kind, bf16, L, W.pads(L)[1]) for L in W.LS)


@pytest.mark.parametrize("kind", KINDS)
def test_a_fault_changes_nothing_where_its_rule_says_so(kind):
    """`fault_applies` may not hide a failure: where it is False, the emulation with the fault returns the fault-free bits"""
    for fault in W.FAULTS[kind]:
        for bf16 in (False, True):
            for L in W.LS:
                L_pad = W.pads(L)[0]
                if W.fault_applies(fault, kind, bf16, L, L_pad):
                    continue
                for fam in (W.FAMILIES[kind][0], "gauss"):
                    c = W.case(kind, fam, L)
                    lens = _lens_list(kind, L)[0]
                    assert np.array_equal(W.emulate(c, bf16, L_pad, lens, fault), W.emulate(c, bf16, L_pad, lens)), (fault, bf16, L)


def test_precision_faults_are_outside_what_the_bound_sees():
    """p_truncated and diag_p_rounded_to_bf16 are not faults the probes must reject.  On record: the causal bound sees neither; the
    relbias bound sees a truncated P in the gauss family only, at some L, by less than a tenth of the bound"""
    worst = {}
    for kind in KINDS:
        for fault in W.PRECISION_FAULTS[kind]:
            for L in W.LS:
                for fam in W.FAMILIES[kind]:
                    c = W.case(kind, fam, L)
                    for lens in _lens_list(kind, L):
                        r = W.reference(c, lens)
                        out = W.emulate(c, True, W.pads(L)[1], lens, fault)
                        assert W.exact_mismatch(out, r) == 0
                        key = (kind, fault, fam.split("_")[0])
                        worst[key] = max(worst.get(key, 0.0), W.worst_ratio(out, *r["bf16"]))
    print("largest |error| / bound with a precision fault:", {k: round(v, 3) for k, v in worst.items()})
    for (kind, fault, group), ratio in worst.items():
        if (kind, fault, group) == ("relbias", "p_truncated", "gauss"):
            assert ratio <= 2.0       # truncation: at most one ulp of bf16 per probability, 2 ub A; the bound holds ub A for P
        else:
            assert ratio <= 1.0, (kind, fault, group, ratio)


# ---------------------------------------------------------------------------------------------------------------------------------
# row operators
# ---------------------------------------------------------------------------------------------------------------------------------
def _ratio(got, ref, bound):
    got = np.asarray(got, np.float64)
    return float("inf") if not np.isfinite(got).all() else float((np.abs(got - ref) / bound).max())


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_rmsnorm_emulation_and_its_faults(bf16):
    worst = 0.0
    for D in W.RMSNORM_DS:
        for M in W.RMSNORM_MS:
            x, w, eps = W.rmsnorm_case(D, M)
            ref = RT.rmsnorm(x, w, eps)
            bound = RT.rmsnorm_bound(ref, D, bf16)
            clean = _ratio(W.emulate_rmsnorm(x, w, eps, bf16), ref, bound)
            assert clean <= 1.0, (D, M, clean)
            worst = max(worst, clean)
            for fault in W.ROW_FAULTS["rmsnorm"]:
                out = W.emulate_rmsnorm(x, w, eps, bf16, fault)
                if W.row_fault_applies(fault, D):
                    assert _ratio(out, ref, bound) > 1.0, (fault, D, M)
                else:
                    assert np.array_equal(out, W.emulate_rmsnorm(x, w, eps, bf16)), (fault, D, M)
    assert sum(W.row_fault_applies("mean_over_padded_width", D) for D in W.RMSNORM_DS) >= 3
    print(f"largest |error| / bound of the fault-free rmsnorm emulation, {DT[bf16]}: {worst:.3f}")


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_geglu_and_gelu_emulations_and_their_faults(bf16):
    for M, F in W.GEGLU_SHAPES:
        u = W.geglu_case(M, F)
        ref, bound = RT.geglu(u, F), RT.geglu_bound(u, F, bf16)
        assert _ratio(W.emulate_geglu(u, F, bf16), ref, bound) <= 1.0, (M, F)
        for fault in W.ROW_FAULTS["geglu"]:
            assert _ratio(W.emulate_geglu(u, F, bf16, fault), ref, bound) > 1.0, (fault, M, F)
    for M, F in W.GELU_SHAPES:
        u = W.gelu_case(M, F)
        for kind in ("erf", "quick"):
            ref, bound = RC.gelu(u, kind), RC.gelu_bound(u, kind, bf16)
            assert _ratio(W.emulate_gelu(u, kind, bf16), ref, bound) <= 1.0, (kind, M, F)
            assert _ratio(W.emulate_gelu(u, kind, bf16, "kinds_swapped"), ref, bound) > 1.0, (kind, M, F)


def _split_matches(outs, want, kinds, tokens):
    """bit for bit inside [0, tokens), and the padding still holds what it held (NaN in the emulation)"""
    for o, w, kind in zip(outs, want, kinds):
        if kind == 0:
            ok = np.array_equal(o, w)
        elif kind == 1:
            ok = np.array_equal(o[:, :, :tokens], w) and np.isnan(o[:, :, tokens:]).all()
        else:
            ok = np.array_equal(o[..., :tokens], w) and np.isnan(o[..., tokens:]).all()
        if not ok:
            return False
    return True


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("kinds", [(0, 1, 2), (2, 0, 1)], ids=["QKV", "VQK"])
def test_split_heads_emulation_and_its_faults(kinds, bf16):
    s = W.SPLIT_SHAPE
    u = W.split_case(kinds)
    want = RC.split_heads(u, s["heads"], s["tokens"], len(kinds), 0.125, kinds)
    want = [W.bf16_round(w) for w in want] if bf16 else want
    args = (u, s["heads"], s["tokens"], s["tokens_pad"], kinds, 0.125, bf16)
    assert _split_matches(W.emulate_split_heads(*args), want, kinds, s["tokens"])
    for fault in W.ROW_FAULTS["split_heads"]:
        assert not _split_matches(W.emulate_split_heads(*args, fault), want, kinds, s["tokens"]), fault
