"""The probes of pmhip_attention_maps can fail: on the CPU, against a float32 numpy restatement of the kernels' arithmetic
(tests/attnmap_ref.py), at the very inputs tests/test_gpu_attention_maps.py runs (B = 2, Nq = 80, heads = 3, the four forms, both
score units, dim_head 64 and 32, Nkv 1 / 33 / 77 / 129 / 416, sigma 2 and 8).

The fault-free restatement stays far inside the element-wise bound; the same restatement with ONE fault -- the last key dropped, the
keys shifted by one, the next query's row, one head left out, division by heads - 1, the two images swapped, and per form a weight
ignored, the first padding key included, a denied segment included -- is rejected wherever the fault exists, and so is `accumulate`
overwriting.  The exact family is bit-exact in the restatement in every form."""
import numpy as np
import pytest

import attnmap_ref as M

SIGMAS = (2.0, 8.0)
_CACHE = {}


def case(form, nkv, dh, sigma, exp2):
    """inputs + float64 reference + bound, computed once, shared and never modified"""
    key = (form, nkv, dh, sigma, exp2)
    if key not in _CACHE:
        d = M.gauss_case(form, nkv, dh, sigma=sigma)
        ref, p, s = M.reference(d["q"], d["k"][:, :, :nkv], d["ok"], d["lay"]["w"], exp2)
        d.update(ref=ref, p=p, s=s, B=M.bound(d["q"], d["k"][:, :, :nkv], ref, p, s, exp2))
        for x in d.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _CACHE[key] = d
    return _CACHE[key]


@pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
@pytest.mark.parametrize("dh", [64, 32])
@pytest.mark.parametrize("form", M.FORMS)
def test_the_restatement_meets_the_bound_and_every_fault_is_rejected(form, dh, exp2):
    clean, weakest = 0.0, {}
    for nkv in M.NKVS:
        for sigma in SIGMAS:
            d = case(form, nkv, dh, sigma, exp2)
            k = d["k"][:, :, :nkv]
            ratio, idx = M.worst(M.emulate(d["q"], k, d["lay"], exp2), d["ref"], d["B"])
            clean = max(clean, ratio)
            assert ratio < 0.05, (nkv, sigma, ratio, idx)
            # rows sum to 1 over the keys that take part, excluded keys are exactly 0
            out = M.emulate(d["q"], k, d["lay"], exp2)
            assert (out[~d["ok"]] == 0).all() and np.isfinite(out).all()
            assert (np.abs(out.astype(np.float64).sum(-1) - 1.0) <= d["B"].sum(-1)).all()
            faults = list(M.FAULTS) + ([M.FORM_FAULTS[form]] if form in M.FORM_FAULTS else [])
            for fault in faults:
                if not M.fault_applies(fault, d["lay"], 2, 80, nkv, 3):
                    continue
                r, _ = M.worst(M.emulate(d["q"], k, d["lay"], exp2, fault=fault), d["ref"], d["B"])
                weakest[fault] = min(weakest.get(fault, np.inf), r)
    print(f"{form} dim_head {dh} exp2={exp2}: clean err / B {clean:.4f}; weakest rejection per fault",
          {f: float(f"{r:.3g}") for f, r in weakest.items()})
    assert all(r > 100.0 for r in weakest.values()), weakest
    assert set(M.FAULTS) <= set(weakest)


@pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
def test_accumulate_is_held_by_the_bound_and_overwriting_is_rejected(exp2):
    for form in M.FORMS:
        d = case(form, 77, 64, 2.0, exp2)
        k = d["k"][:, :, :77]
        half = M.emulate(d["q"], k, d["lay"], exp2, scale=0.5)
        both = M.emulate(d["q"], k, d["lay"], exp2, scale=0.5, into=half)
        Bd = 2 * M.bound(d["q"], k, d["ref"], d["p"], d["s"], exp2, scale=0.5, accumulate_out=both)
        assert M.worst(both, d["ref"], Bd)[0] < 0.05
        wrong = M.emulate(d["q"], k, d["lay"], exp2, scale=0.5, into=half, fault="accumulate_overwrites")
        assert M.worst(wrong, d["ref"], Bd)[0] > 100.0


@pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
@pytest.mark.parametrize("dh", [64, 32])
def test_the_exact_family_is_bit_exact(dh, exp2):
    for form in M.FORMS:
        for nkv in M.NKVS:
            lay = M.layout(form, 2, 80, nkv)
            ok = M.allowed(lay, 2, 80, nkv)
            q, k, expect = M.exact_inputs(2, 4, 80, nkv, dh, ok)
            assert np.array_equal(M.emulate(q, k, lay, exp2), expect), (form, nkv)
            assert np.array_equal(expect.sum(-1), np.ones((2, 80), np.float32)) and (expect[~ok] == 0).all()
            ref, _, _ = M.reference(q, k, ok, lay["w"], exp2)
            assert np.abs(ref - expect).max() < 1e-15
            half = M.emulate(q, k, lay, exp2, scale=0.5)
            assert np.array_equal(M.emulate(q, k, lay, exp2, scale=0.5, into=half), expect)
            for fault in ("shift_keys", "swap_images", "skip_head"):
                if nkv > 1:
                    assert not np.array_equal(M.emulate(q, k, lay, exp2, fault=fault), expect), (form, nkv, fault)


def test_the_layouts_are_what_the_docstrings_say():
    for nkv in M.NKVS:
        for form in M.FORMS:
            lay = M.layout(form, 2, 80, nkv)
            ok = M.allowed(lay, 2, 80, nkv)
            assert ok.any(-1).all() and ok[:, :, 0].all()
            if nkv > 5:
                assert form == "plain" or not ok.all()
        seg = M.layout("segments", 2, 80, nkv)
        assert set(np.unique(seg["ks"])) <= {0, 1, 2, M.PAD}
        w = M.layout("weighted", 2, 80, nkv)["w"]
        assert set(np.unique(w)) <= set(M.WEIGHTS.tolist())
    assert set(np.unique(M.layout("weighted", 2, 80, 416)["w"])) == set(M.WEIGHTS.tolist())
    kp = M.gauss_case("segments", 77, 64)["k"]
    assert kp.shape[2] == 128 and np.isnan(kp[:, :, 77:]).all() and np.isnan(kp[:, :, 4]).all() and np.isfinite(kp[:, :, 0]).all()
