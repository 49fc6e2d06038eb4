"""The attention probes can fail: on the CPU, against a numpy restatement of the bf16 kernel's arithmetic.

The fault-free restatement meets the element-wise bound of tests/attention_probes.py in every family at every key count of the
edge list, in both modes; the same restatement with ONE index fault (a dropped key, an included padding key, two V rows
exchanged, an 8-key chunk of V^T read late, a result stored one query row off) is rejected by at least one family at every key
count where the fault exists.  tests/test_gpu_attention_probes.py holds the kernels to exactly these checks.

truncate_p (P truncated to bf16 instead of rounded) is NOT in the list of faults that must be rejected.  The gauss family at
sigma = 4 was meant to reject it from 64 keys on, and it does not: largest err / B over those key counts in exp2 mode 0.66 with
truncation, 0.47 without (the reason is with attention_probes.INDEX_FAULTS).  Nothing was loosened for it;
test_truncated_p_is_outside_what_the_bound_sees records the fact.
"""
import numpy as np
import pytest

import attention_probes as P


def _families(nkv, exp2):
    """name -> data; small query counts (the selector: Nq = Nkv, two (batch, head) with their own codes and permutations)"""
    return {"selector": P.selector((2,), nkv, exp2), "uniform": P.uniform((1,), 3, nkv), "gauss0.3": P.gauss((1,), 48, nkv, 0.3),
            "gauss4": P.gauss((1,), 48, nkv, 4.0)}


_CACHE = {}


def _case(nkv, exp2):
    """families + their float64 reference and bound, computed once and shared by the tests below (never modified)"""
    if (nkv, exp2) not in _CACHE:
        fams = _families(nkv, exp2)
        for d in fams.values():
            ref, A, s = P.reference(d["q"], d["k"], d["v"], exp2)
            d.update(ref=ref, s=s, B=P.bound("bf16", ref, A, P.score_error(d["q"], d["k"], s, exp2), nkv))
            for x in d.values():
                if isinstance(x, np.ndarray):
                    x.setflags(write=False)
        _CACHE[nkv, exp2] = fams
    return _CACHE[nkv, exp2]


def _rejected(name, d, out):
    ratio, _ = P.worst_ratio(out, d["ref"], d["B"])
    return ratio > 1.0 or (name == "selector" and not np.array_equal(out, d["expect"]))


def test_helpers():
    x = np.array([1.0, 1.00390625, 1.01171875, -3.0e38, 0.0, 2.0 ** -130], np.float32)       # ties go to even
    assert np.array_equal(P.bf16_round(x)[:3], np.array([1.0, 1.0, 1.015625], np.float32)) and P.is_bf16(P.bf16_round(x))
    assert np.array_equal(P.bf16_trunc(x)[:3], np.array([1.0, 1.0, 1.0078125], np.float32))
    v = P.selector_values(np.arange(3)[:, None, None], np.arange(512)[None, :, None], np.arange(64)[None, None, :])
    assert P.is_bf16(v) and np.abs(v).min() >= 1 and np.abs(v).max() < 4
    assert all(len(np.unique(v[b, :, d])) == 512 for b in range(3) for d in (0, 63)) and len(np.unique(v[0, 5])) == 64
    o = np.arange(2 * 3 * 5 * 4, dtype=np.float32).reshape(2, 3, 5, 4)
    assert np.array_equal(P.from_out_layout(P.out_layout(o), 2, 3, 5, 4), o) and P.out_layout(o)[5 + 2, 4 + 1] == o[1, 1, 2, 1]
    ratio, msg = P.check_bound(np.array([[[1.0, np.nan]]]), np.ones((1, 1, 2)), np.ones((1, 1, 2)), np.zeros((1, 1, 3)), "x")
    assert ratio == np.inf and "(0, 0, 1)" in msg and "largest-weight key is 0 of 3" in msg
    assert P.worst_ratio(np.zeros(2), np.zeros(2), np.zeros(2))[0] == 0.0              # exact zeros under a zero bound pass


@pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
def test_fault_free_emulation_meets_the_bound(exp2):
    worst = {}
    for nkv in P.EDGE_NKV:
        fams = _case(nkv, exp2)
        sel, uni = fams["selector"], fams["uniform"]
        # the selector's conditions: float64 off-target mass <= 2^-12 in every row, and no fallback due (l < 2^60)
        mass, log2_l = P.selector_conditions(sel["codes"], sel["c"], exp2)
        assert mass <= 2.0 ** -12 and log2_l <= 60.0, (nkv, mass, log2_l)
        assert np.array_equal(sel["s"].argmax(-1), sel["target"]) and np.abs(sel["ref"] - sel["expect"]).max() <= 2.0 ** -12 * 8
        assert sorted(sel["target"][0].tolist()) == list(range(nkv)) and (nkv == 1 or not np.array_equal(sel["target"][0], sel["target"][1]))
        # the uniform probe's: every probability 1 / Nkv, the reference is count_d / Nkv
        count = np.bincount(np.arange(nkv) % 64, minlength=64)
        assert np.allclose(uni["ref"][0, 0], count / nkv, rtol=1e-13, atol=0) and not uni["q"].any()
        for name, d in fams.items():
            assert all(P.is_bf16(d[x]) for x in "qkv")
            out = P.emulate_bf16(d["q"], d["k"], d["v"], exp2)
            ratio, msg = P.check_bound(out, d["ref"], d["B"], d["s"], f"{name} Nkv={nkv}")
            assert msg is None, msg
            worst[name] = max(worst.get(name, 0.0), ratio)
            if name == "selector":
                assert np.array_equal(out, d["expect"]), nkv
    print("largest err / B of the fault-free emulation:", {k: round(v, 3) for k, v in worst.items()})
    assert worst["gauss4"] > 0.2                                 # the bound is not slack by an order of magnitude either


@pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
@pytest.mark.parametrize("fault", P.INDEX_FAULTS)
def test_every_index_fault_is_rejected_at_every_key_count(fault, exp2):
    applies = 0
    for nkv in P.EDGE_NKV:
        if not P.fault_applies(fault, nkv, nkv):
            continue
        applies += 1
        by = [name for name, d in _case(nkv, exp2).items() if _rejected(name, d, P.emulate_bf16(d["q"], d["k"], d["v"], exp2, fault))]
        assert by, f"{fault} at Nkv={nkv} passes every family"
    assert applies >= 16, applies
    print(f"{fault}: rejected at all {applies} key counts where it applies")


def test_truncated_p_is_outside_what_the_bound_sees():
    """Recorded, not required (module docstring): truncation moves the result, but by less than the bound grants rounding."""
    ratios = []
    for nkv in [x for x in P.EDGE_NKV if x >= 64]:
        d = _case(nkv, True)["gauss4"]
        good, bad = (P.emulate_bf16(d["q"], d["k"], d["v"], True, f) for f in (None, "truncate_p"))
        assert not np.array_equal(good, bad)
        ratios.append(P.worst_ratio(bad, d["ref"], d["B"])[0])
    print("largest err / B with P truncated:", round(max(ratios), 3))
    assert max(ratios) <= 1.0                                    # if this ever fails, truncate_p belongs in INDEX_FAULTS
