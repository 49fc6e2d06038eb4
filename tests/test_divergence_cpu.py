"""Mask-free editing without a GPU.

(a) the bound of tests/divergence_ref.py rejects every named fault at exactly the inputs tests/test_gpu_divergence.py launches while the
float32 restatements pass; (b) ``diff_draws``; (c) the CPU branch of ``diff_mask`` / ``diff_edit`` on the tiny pipelines and the
composition with the pair loop; (d) the setting the GPU file compares against this branch, shown here -- in float64, on this branch's
own logits -- to keep every token's score further from the region's cut than the GPU tolerance can move it; (e) the new symbol, the
header, the prototypes and the ABI version; (f) the argument faults."""
import math
import os
import re

import numpy as np
import pytest
import torch

import divergence_ref as R
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline, diff_draws
from test_control_cpu import LENS_EDIT, LENS_SRC, PAIRS, _tiny, pair_case
from test_forced_cpu import t5_pipe
from util import ROOT

TOL = 1e-3                                  # the project's float bar (tests/test_gpu_control.py): the gap granted between the two branches' logits
SCORE_REL = math.expm1(2 * TOL)             # eps: a logit within TOL moves a probability by at most expm1(2 TOL) of itself
IMG_SEED = 4
# the settings the GPU file compares against this branch: chosen here, on the CPU, by the margins test below (a scan over 160 draw
# seeds x thresholds 0.70 .. 0.99 on this branch alone)
SETTING = {"tv": dict(seed=22, threshold=0.95), "jeffreys": dict(seed=44, threshold=0.88)}
AUDIT_CAP = 0                               # no position of the GPU's mask may differ from this branch's


def jeffreys_tol(R_max):
    """what the float bar grants a jeffreys score.  The two branches' logits differ by at most TOL, so log p moves by at most 2 TOL
    and p by at most eps = expm1(2 TOL) of itself.  A term (p - q)(log p - log q) then moves by at most
    (eps p + eps q) (|L| + 4 TOL) + |p - q| 4 TOL, L = log p - log q; summed over the columns, with sum p = sum q = 1, sum |p - q| <= 2
    and |L| <= R = max |log p - log q|:  2 eps (R + 4 TOL) + 8 TOL.  (tv: 1/2 sum (eps p + eps q) = eps.)"""
    return 2 * SCORE_REL * (R_max + 4 * TOL) + 8 * TOL


@pytest.fixture(scope="module")
def pipe():
    return _tiny()


def photo(pipe, B=PAIRS):
    S = pipe.image_size
    return torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(IMG_SEED)) * 2 - 1


def setting_call(pipe, kind, device=None, **kw):
    """``diff_mask`` at the margins test's setting: the two contexts of ``pair_case`` under their lengths -> (mask, score)"""
    src, edit, *_ = pair_case(pipe)
    img = photo(pipe)
    if device is not None:
        src, edit, img = src.to(device), edit.to(device), img.to(device)
    return pipe.diff_mask(img, src, edit, kind=kind, context_lens=LENS_SRC, edit_context_lens=LENS_EDIT, return_score=True, **SETTING[kind], **kw)


# ------------------------------------------------------------------------------------------------------------- (a) the bound

def launches(V):
    """every (case, accumulate) the GPU file launches at this V, with its float64 reference and bound"""
    for kind in R.KINDS:
        for variant in (0, 1):
            d = R.case(V, kind, variant)
            for accumulate in (False, True):
                kw = dict(acc0=d["acc0"], count0=d["count0"], accumulate=accumulate)
                yield d, kw, R.reference(d["a"], d["b"], d["ids"], V, kind, **kw), R.bound(d["a"], d["b"], kind, d["acc0"] if accumulate else None)


@pytest.mark.parametrize("V", R.VS)
def test_the_bound_rejects_every_named_fault_at_the_gpu_tests_inputs(V):
    rejected = {f: 0 for f in R.FAULTS}
    worst_f32 = 0.0
    for d, kw, want, B in launches(V):
        assert R.check(want[:2], want, B) == ([], 0.0)
        a, b = (torch.from_numpy(np.array(d[k])) for k in ("a", "b"))
        for f32 in (R.restate_f32(d["a"], d["b"], d["kind"]), Pipeline._divergence_cpu(a, b, d["kind"]).numpy()):
            assert f32.dtype == np.float32
            acc = (d["acc0"] + f32 if kw["accumulate"] else f32).astype(np.float32)
            acc = np.where(want[2], acc, d["acc0"] if kw["accumulate"] else np.float32(0))
            fails, worst = R.check((acc, want[1]), want, B)
            worst_f32 = max(worst_f32, worst)
            assert not fails, fails
        for fault in R.FAULTS:
            got = R.reference(d["a"], d["b"], d["ids"], V, d["kind"], fault=fault, **kw)
            rejected[fault] += len(R.check(got[:2], want, B)[0])
    print(f"V={V}: the float32 restatements' worst err / bound {worst_f32:.4f}; rows on which each fault is rejected: {rejected}")
    assert all(v > 0 for v in rejected.values()), rejected


def test_the_inputs_are_what_the_docstring_says():
    for V in R.VS:
        seen = np.zeros(R.M, int)
        for variant in (0, 1):
            d = R.case(V, "tv", variant)
            a, b, ids = d["a"], d["b"], d["ids"]
            assert all(np.array_equal(d[k], R.case(V, "jeffreys", variant)[k], equal_nan=True) for k in ("a", "b", "ids"))
            assert a.shape == b.shape == (R.M, V) and a.dtype == b.dtype == np.float32 and R.M == 9
            seen += ids == V
            assert ((ids >= 0) & (ids <= V)).all()
            tv, je = R.divergence(a, b, "tv"), R.divergence(a, b, "jeffreys")
            assert np.array_equal(a[0], b[0]) and tv[0] == 0.0 and je[0] == 0.0
            assert np.array_equal(b[1], a[1] + np.float32(R.SHIFT)) and tv[1] < 1e-5
            last = max((R.layout(V, k)[0] - 1) * R.layout(V, k)[1] * 256 for k in R.KINDS)         # where the last register group starts
            assert int(a[2].argmax()) == V - 2 >= last and a[2].max() - np.delete(a[2], V - 2).max() > 90 and int(b[2].argmax()) != V - 2
            assert a[2].max() - b[2].max() > 104 and tv[2] > 0.99                  # (a shared maximum: exp(-104) is below every float32)
            assert (a[3].max() - a[3].min() < 0.5) and 1e-4 < tv[3] < 0.05
            assert int(a[4].argmax()) == int(b[4].argmax()) and 1e-3 < tv[4] < 0.95
            assert np.isneginf(a[5, 9]) and np.isneginf(b[5, 9]) and np.isfinite(tv[5]) and np.isfinite(je[5])
            assert np.isneginf(a[6, 9]) and np.isfinite(b[6, 9]) and np.isfinite(tv[6]) and je[6] == np.inf
            assert np.isnan(b[7]).sum() == 1 and not np.isnan(a[7]).any() and np.isnan(tv[7]) and np.isnan(je[7])
            assert np.isnan(a[8]).all() and np.isnan(b[8]).all()
        assert (seen == 1).all()                                                   # every row is scored once and skipped once
    assert [R.layout(V, "tv") for V in R.VS] == [(1, 1), (4, 1), (8, 4), (8, 8)] and 1000 % 64 and 1000 % 256
    assert [R.layout(V, "jeffreys") for V in R.VS] == [(1, 1), (4, 1), (4, 8), (4, 16)]


# ------------------------------------------------------------------------------------------------------------- (b) the draws

def test_diff_draws():
    for B, N, ratio, draws in ((2, 16, 0.5, 4), (3, 256, 0.5, 4), (1, 17, 0.3, 5), (2, 16, 0.999, 1), (2, 10, 0.25, 4)):
        m = diff_draws(B, N, ratio, draws, 7)
        k = math.ceil(ratio * N)
        assert m.dtype == torch.bool and tuple(m.shape) == (draws, B, N) and m.device.type == "cpu"
        assert (m.sum(-1) == k).all()                                              # every draw masks exactly k per image
        assert (m.sum(0) >= 1).all()                                               # every position is masked in at least one draw
        assert torch.equal(m, diff_draws(B, N, ratio, draws, 7))
        if N > 10 and draws > 1:
            assert not torch.equal(m, diff_draws(B, N, ratio, draws, 8))
    assert (diff_draws(2, 16, 0.5, 4, 0).sum(0) == 2).all()                         # the tiny pipeline's 16 tokens at the defaults: exactly 2
    rank = torch.argsort(torch.argsort(torch.rand(2, 16, generator=torch.Generator().manual_seed(3)), dim=1), dim=1)
    assert torch.equal(diff_draws(2, 16, 0.5, 4, 3)[1], (rank - 4) % 16 < 8)        # the rule, restated
    with pytest.raises(ValueError, match=r"k >= ceil\(N / draws\)"):
        diff_draws(2, 16, 0.2, 3, 0)                                               # k = 4 < ceil(16 / 3) = 6
    with pytest.raises(ValueError, match=r"k >= ceil\(N / draws\)"):
        diff_draws(2, 16, 0.5, 1, 0)
    for bad in (dict(mask_ratio=0.0), dict(mask_ratio=1.0), dict(mask_ratio=-0.5), dict(mask_ratio="0.5"), dict(draws=0), dict(draws=2.0),
                dict(draws=True), dict(seed=1.5), dict(B=0), dict(N=0)):
        kw = dict(B=2, N=16, mask_ratio=0.5, draws=4, seed=0)
        kw.update(bad)
        with pytest.raises(ValueError, match="diff_draws"):
            diff_draws(**kw)


# ------------------------------------------------------------------------------------------------------------- (c) the CPU branch

def test_identical_prompts_give_a_zero_score_and_an_empty_mask(pipe):
    src, *_ = pair_case(pipe)
    g = pipe.image_size // pipe.patch_size
    for kind in R.KINDS:
        mask, score = pipe.diff_mask(photo(pipe), src, src, kind=kind, context_lens=LENS_SRC, edit_context_lens=LENS_SRC, return_score=True)
        assert mask.dtype == torch.bool and tuple(mask.shape) == (PAIRS, g, g) and score.dtype == torch.float32 and tuple(score.shape) == (PAIRS, g, g)
        assert bool((score == 0).all()) and not bool(mask.any())
    t5 = t5_pipe()
    mask, score = t5.diff_mask(photo(t5), ["a red barn", "the cow"], ["a red barn", "the cow"], mask_padding=True, return_score=True)
    assert bool((score == 0).all()) and not bool(mask.any())
    one = t5.diff_mask(photo(t5), "a red barn", "a red barn")                      # a single prompt for every image
    assert tuple(one.shape) == (PAIRS, g, g) and not bool(one.any())


def test_different_prompts_give_a_region_and_the_rule_is_the_docstrings(pipe):
    g, N, V = pipe.image_size // pipe.patch_size, pipe.num_tokens, pipe.mask_token_id
    for kind in R.KINDS:
        mask, score = setting_call(pipe, kind, grow=0)
        assert 0 < int(mask.sum()) < mask.numel() and bool((score > 0).all())
        again, _ = setting_call(pipe, kind, grow=0)
        assert torch.equal(mask, again)
        grown, same_score = setting_call(pipe, kind, grow=1)
        assert torch.equal(score, same_score) and bool((grown | ~mask).all()) and int(grown.sum()) > int(mask.sum())
        assert torch.equal(grown, torch.nn.functional.max_pool2d(mask[:, None].float(), 3, stride=1, padding=1)[:, 0] > 0)
        # the rule, restated from the operator level of this branch
        src, edit, *_ = pair_case(pipe)
        ids = pipe.to_latent(photo(pipe))[1].reshape(PAIRS, N)
        acc, count = torch.zeros(PAIRS, N), torch.zeros(PAIRS, N)
        for m in diff_draws(PAIRS, N, 0.5, 4, SETTING[kind]["seed"]):
            masked = torch.where(m, torch.full_like(ids, V), ids)
            with torch.no_grad():
                la = pipe.tokens2logits(pipe.ids2tokens(masked), src, context_lens=LENS_SRC)
                lb = pipe.tokens2logits(pipe.ids2tokens(masked), edit, context_lens=LENS_EDIT)
            acc += torch.where(m, Pipeline._divergence_cpu(la, lb, kind), torch.zeros(()))
            count += m
        want = (acc / count).reshape(PAIRS, g, g)
        assert float((score - want).abs().max()) < 1e-5                            # (one forward of 2 B images against two of B)
        assert torch.equal(mask, score >= SETTING[kind]["threshold"] * score.amax(dim=(1, 2), keepdim=True))
    t5 = t5_pipe()
    mask = t5.diff_mask(photo(t5), ["a red barn", "the cow"], ["a red church", "the big cow"], mask_padding=True, threshold=0.9, grow=0)
    assert 0 < int(mask.sum()) < mask.numel()


def test_diff_edit_is_its_two_calls_and_edit_keeps_what_is_outside(pipe):
    t5 = t5_pipe()
    N, V = t5.num_tokens, t5.mask_token_id
    img = photo(t5)
    text, edit = ["a red barn", "the cow"], ["a red church", "the big cow"]
    kw = dict(threshold=0.9, grow=0, kind="tv", mask_ratio=0.5, draws=4)
    ekw = dict(timesteps=3, seed=5, return_ids=True, mask_padding=True)
    (out, ids), mask = t5.diff_edit(img, text, edit, diff_seed=3, return_mask=True, **kw, **ekw)
    by_hand_mask = t5.diff_mask(img, text, edit, seed=3, mask_padding=True, **kw)
    by_hand, by_hand_ids = t5.edit(img, token_mask=by_hand_mask, text=edit, **ekw)
    assert torch.equal(mask, by_hand_mask) and torch.equal(ids, by_hand_ids) and torch.equal(out, by_hand)      # bit for bit
    assert 0 < int(mask.sum()) < mask.numel()
    s = t5.to_latent(img)[1].reshape(PAIRS, N)
    outside = ~mask.reshape(PAIRS, N)
    assert torch.equal(ids[outside], s[outside]) and not bool((ids == V).any())    # edit keeps every token outside the mask
    plain = t5.diff_edit(img, text, edit, diff_seed=3, **kw, **ekw)
    assert torch.equal(plain[0], out) and torch.equal(plain[1], ids)
    # an image whose prompts agree comes back as edit returns an empty mask: decode(encode(img))
    same, same_mask = t5.diff_edit(img, text, text, return_mask=True, timesteps=2, seed=5)
    assert not bool(same_mask.any()) and torch.equal(same, t5.vqgan.decode_from_indice(s))
    for bad in (dict(mask=mask), dict(token_mask=mask)):
        with pytest.raises(ValueError, match="diff_edit"):
            t5.diff_edit(img, text, edit, **bad)


def test_the_mask_serves_the_pair_loop_on_a_photograph():
    t5 = t5_pipe()
    N, V = t5.num_tokens, t5.mask_token_id
    img = photo(t5)
    text, edit = ["a red barn", "the cow"], ["a red church", "the big cow"]
    mask = t5.diff_mask(img, text, edit, mask_padding=True, threshold=0.9, grow=0)
    ids_s, ids_e = t5.prompt_to_prompt(text, edit, img=img, blend_mask=mask, blend_start=0.0, mode="replace", timesteps=3, seed=5, return_ids=True)
    s = t5.to_latent(img)[1].reshape(PAIRS, N)
    outside = ~mask.reshape(PAIRS, N)
    assert bool(((ids_e[outside] == s[outside]) | (ids_e[outside] == V)).all())    # outside the mask the edited half keeps the photograph's tokens
    assert bool(((ids_s == s) | (ids_s == V)).all())


# ------------------------------------------------------------------------------------------------------------- (d) the GPU file's inputs

def scores_in_float64(pipe, kind):
    """the setting's score recomputed in float64 from this branch's own logits -> (score64 [B, N], R = max |log p - log q| over the
    compared rows, the branch's mask and score)"""
    N, V = pipe.num_tokens, pipe.mask_token_id
    seen, real = [], pipe._divergence_cpu
    pipe._divergence_cpu = lambda la, lb, k: (seen.append((la.double().numpy(), lb.double().numpy())), real(la, lb, k))[1]
    try:
        mask, score = setting_call(pipe, kind)
    finally:
        del pipe._divergence_cpu
    masks = diff_draws(PAIRS, N, 0.5, 4, SETTING[kind]["seed"]).numpy()
    assert len(seen) == len(masks) == 4
    acc, count, r_max = np.zeros((PAIRS, N)), np.zeros((PAIRS, N)), 0.0
    for m, (la, lb) in zip(masks, seen):
        acc += np.where(m, R.divergence(la.reshape(-1, V), lb.reshape(-1, V), kind).reshape(PAIRS, N), 0.0)
        count += m
        lp, lq = (x - x.max(-1, keepdims=True) - np.log(np.exp(x - x.max(-1, keepdims=True)).sum(-1, keepdims=True)) for x in (la, lb))
        r_max = max(r_max, float(np.abs(lp - lq)[m].max()))
    return acc / count, r_max, mask, score


@pytest.mark.parametrize("kind", R.KINDS)
def test_the_setting_the_gpu_file_compares_is_far_from_a_tie(pipe, kind):
    """the GPU file holds the fp32 engine's mask to this branch's with no differing position (AUDIT_CAP).  Here the setting is shown
    to keep every token's float64 score further from threshold * max than the GPU tolerance can move the two of them."""
    score64, r_max, mask, score = scores_in_float64(pipe, kind)
    thr = SETTING[kind]["threshold"]
    tol = SCORE_REL if kind == "tv" else jeffreys_tol(r_max)
    cut = thr * score64.max(1, keepdims=True)
    margin = float((np.abs(score64 - cut) / (tol * (1 + thr))).min())
    print(f"{kind}: R = {r_max:.3f}, tolerance {tol:.3e}, the closest score is {margin:.2f} x the tolerance of both sides from the cut")
    assert margin > 1.0, "a score lies within the GPU tolerance of the cut: widen the scan over seeds"
    assert float(np.abs(score.reshape(PAIRS, -1).double().numpy() - score64).max()) < 1e-5
    g = pipe.image_size // pipe.patch_size
    region = torch.from_numpy(score64 >= cut).reshape(PAIRS, 1, g, g)
    assert torch.equal(mask, torch.nn.functional.max_pool2d(region.float(), 3, stride=1, padding=1)[:, 0] > 0)
    again = setting_call(pipe, kind)[0]
    assert int((again != mask).sum()) <= AUDIT_CAP and 0 < int(mask.sum()) < mask.numel()


# ------------------------------------------------------------------------------------------------------------- (e) the ABI

def test_the_new_symbol_the_header_and_the_prototypes():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "pmhip.h")).read()
    m = re.search(r"int pmhip_logit_divergence\(([^;]*)\);", hdr)
    assert m, "pmhip_logit_divergence is not declared in include/pmhip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    kinds = ["ptr" if "*" in p else p.split()[0] for p in params[:-1]] + ["ptr"]   # (pmhip_stream is a pointer)
    assert kinds == ["ptr", "ptr", "int", "ptr", "int64_t", "int", "ptr", "ptr", "int", "int", "int", "ptr"]
    as_kind = {C.c_void_p: "ptr", C.c_int: "int", C.c_int64: "int64_t"}
    res, argtypes = _lib.PROTOTYPES["pmhip_logit_divergence"]
    assert res is C.c_int and [as_kind[a] for a in argtypes] == kinds
    assert re.search(r"#define PMHIP_ABI_VERSION 11\b", hdr) and _lib.ABI_VERSION == 11
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11 and hasattr(lib, "pmhip_logit_divergence")


def test_the_entry_refuses_before_it_launches():
    """every PMHIP_EINVAL of the entry returns in front of the launch: dummy pointers, no GPU"""
    import ctypes as C
    lib = _lib.load()
    p = C.c_void_p(64)

    def rc(a=p, b=p, ldl=72, ids=p, kind=0, acc=p, count=p, accumulate=0, M=9, V=64):
        return lib.pmhip_logit_divergence(a, b, ldl, ids, 64, kind, acc, count, accumulate, M, V, None)
    for bad, text in ((dict(a=None), b"a is NULL"), (dict(b=None), b"b is NULL"), (dict(acc=None), b"acc is NULL"), (dict(a=C.c_void_p(68)), b"aligned"),
                      (dict(M=0), b"M=0"), (dict(M=-3), b"M=-3"), (dict(V=0), b"V=0"), (dict(V=-4), b"V=-4"), (dict(V=16388, ldl=16388), b"V=16388"),
                      (dict(V=62, ldl=64), b"V=62"), (dict(ldl=70), b"ldl=70"), (dict(ldl=60), b"ldl=60"), (dict(V=1000, ldl=996), b"ldl=996"),
                      (dict(kind=2), b"kind=2"), (dict(kind=-1), b"kind=-1")):
        assert rc(**bad) == _lib.PMHIP_EINVAL, bad
        msg = lib.pmhip_last_error()
        assert b"logit_divergence" in msg and text in msg, (bad, msg)
        assert not re.search(rb"PMHIP_[A-Z0-9_]+", msg)


# ------------------------------------------------------------------------------------------------------------- (f) argument faults

def test_the_operators_argument_faults_are_value_errors():
    a, b = torch.zeros(9, 64), torch.zeros(9, 64)
    ids = torch.full((9,), 64, dtype=torch.int64)
    wide = torch.zeros(9, 72)
    for bad in (dict(a=a.double()), dict(b=b.half()), dict(a=a[0]), dict(a=None), dict(b=b[:8]), dict(b=torch.zeros(9, 68)), dict(a=torch.zeros(9, 62), b=torch.zeros(9, 62)),
                dict(a=torch.zeros(2, 16388), b=torch.zeros(2, 16388)), dict(a=torch.zeros(0, 64), b=torch.zeros(0, 64)),
                dict(a=wide[:, :64], b=b), dict(a=wide[:, 2:66], b=wide[:, 2:66]), dict(a=a.t().contiguous().t(), b=b.t().contiguous().t()),
                dict(a=torch.zeros(9, 70)[:, :64], b=torch.zeros(9, 70)[:, :64]),
                dict(kind="kl"), dict(kind=0), dict(ids=ids), dict(mask_id=64), dict(ids=ids, mask_id=64.0), dict(ids=ids, mask_id=True),
                dict(ids=ids.int(), mask_id=64), dict(ids=ids[:8], mask_id=64), dict(ids=torch.zeros(18, dtype=torch.int64)[::2], mask_id=64),
                dict(accumulate=True)):
        kw = dict(a=a, b=b)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.logit_divergence(**kw)
    with pytest.raises(_lib.PmhipError):                                           # host memory: no CPU fallback
        ops.logit_divergence(a, b)
    with pytest.raises(_lib.PmhipError):
        ops.logit_divergence(wide[:, :64], wide[:, :64], ids=ids, mask_id=64, kind="jeffreys")          # (a common row stride is served)


def test_diff_masks_argument_faults_are_value_errors(pipe):
    src, edit, *_ = pair_case(pipe)
    img = photo(pipe)
    S = pipe.image_size
    ok = dict(img=img, text=src, edit_text=edit)
    for bad in (dict(threshold=0.0), dict(threshold=1.5), dict(threshold="0.5"), dict(threshold=True), dict(grow=-1), dict(grow=1.0), dict(kind="kl"),
                dict(mask_ratio=0.0), dict(mask_ratio=1.0), dict(draws=0), dict(mask_ratio=0.2, draws=3), dict(seed=0.5),
                dict(img=img[0]), dict(img=img[:, :, :S - 8]), dict(img=None), dict(text=None), dict(edit_text=None),
                dict(text=src[:1]), dict(edit_text=edit[:, :40]), dict(edit_text=edit[0]), dict(text=["a"]), dict(text=["a", "b", "c"]), dict(text=[1, 2]),
                dict(text=3.0), dict(mask_padding=True), dict(context_lens=[77]), dict(context_lens=[77, 0]), dict(edit_context_lens=[78, 5]),
                dict(guidance_scale=3.0), dict(negative_text=["x", "y"]), dict(context_segments=np.zeros((2, 77))), dict(context_weights=np.ones((2, 77))),
                dict(prompt_weights=True), dict(regions=[])):
        kw = dict(ok)
        kw.update(bad)
        with pytest.raises(ValueError):
            pipe.diff_mask(**kw)
    assert tuple(pipe.diff_mask(img, ["a", "b"], pipe.text_model(["c", "d"])).shape) == (PAIRS, S // pipe.patch_size, S // pipe.patch_size)    # prompts against a tensor
