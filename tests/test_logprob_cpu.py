"""Model likelihood without a GPU.

(a) tests/logprob_ref.py: its bound rejects each named fault at exactly the inputs tests/test_gpu_logprob.py launches, accepts the
float32 restatements, and the inputs are what its docstring says; (b) the plain-torch branch of ``token_scores`` / ``score`` /
``surprise_mask`` / ``best_of`` on the tiny pipeline against the float64 rule applied to that branch's own logits; (c) the ABI, the
refusals of the entry, of the operator and of the pipeline calls."""
import os
import re

import numpy as np
import pytest
import torch

import logprob_ref as R
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline, TokenScores, best_index, diff_draws
from test_control_cpu import LENS_SRC, PAIRS, _tiny, pair_case
from test_divergence_cpu import photo
from util import ROOT

SCALES = (None, 3.0)


@pytest.fixture(scope="module")
def pipe():
    return _tiny()


# ------------------------------------------------------------------------------------------------------------- (a) the bound

def launches(V):
    """every (case, accumulate) the GPU file launches at this V, with its float64 reference and bound"""
    for variant in R.VARIANTS:
        d = R.case(V, variant)
        for accumulate in (False, True):
            kw = dict(logp0=d["logp0"], ent0=d["ent0"], rank0=d["rank0"], count0=d["count0"], accumulate=accumulate)
            prev = dict(logp0=d["logp0"], ent0=d["ent0"]) if accumulate else {}
            yield d, kw, R.reference(d["a"], d["ids"], V, d["target"], **kw), prev


def stored(d, kw, want, f32):
    """what a launch leaves when its scored rows compute f32 = (lp, ent, rk)"""
    scored = want[4]
    if kw["accumulate"]:
        vals = [(d[k] + v).astype(d[k].dtype) for k, v in zip(("logp0", "ent0", "rank0"), f32)]
        return [np.where(scored, v, d[k]) for v, k in zip(vals, ("logp0", "ent0", "rank0"))] + [want[3]]
    return [np.where(scored, v, np.zeros_like(v)) for v in f32] + [want[3]]


@pytest.mark.parametrize("V", R.VS)
def test_the_bound_rejects_every_named_fault_at_the_gpu_tests_inputs(V):
    rejected = {f: 0 for f in R.FAULTS}
    worst_f32 = 0.0
    for d, kw, want, prev in launches(V):
        assert R.check(want[:4], want, R.bound(d["a"], d["target"], **prev)) == ([], 0.0)
        # the float32 restatements (torch's sums: at most V additions deep) lie within the bound of their own depth
        B = R.bound(d["a"], d["target"], n_adds=V, **prev)
        t = np.where(want[4], d["target"], 0)
        x = np.where(want[4][:, None], d["a"], np.float32(0))               # (an unscored row's NaN: not this evaluation's business)
        cpu = Pipeline._token_logprob_cpu(torch.from_numpy(x), torch.from_numpy(t))
        for f32 in (R.restate_f32(x, t), tuple(v.numpy() for v in cpu)):
            assert f32[0].dtype == np.float32 and f32[1].dtype == np.float32
            fails, worst = R.check(stored(d, kw, want, (f32[0], f32[1], f32[2].astype(np.int32))), want, B)
            worst_f32 = max(worst_f32, worst)
            assert not fails, fails
        B = R.bound(d["a"], d["target"], **prev)
        for fault in R.FAULTS:
            got = R.reference(d["a"], d["ids"], V, d["target"], fault=fault, **kw)
            rejected[fault] += len(R.check(got[:4], want, B)[0])
    print(f"V={V}: the float32 restatements' worst err / bound {worst_f32:.4f}; values on which each fault is rejected: {rejected}")
    if V == 4:                                                               # one float4: no register group to leave out that is not the row
        rejected.pop("last_group_out_of_max")
    assert all(v > 0 for v in rejected.values()), rejected


def test_the_four_named_faults_are_rejected_where_the_docstring_says():
    V = 1024
    for fault, variant, rows in (("neighbouring_column", 2, range(R.M)), ("rank_without_the_column_tie_break", 2, range(1, R.M)),     # (probe row 0: column 0 has none below it)
                                 ("entropy_without_the_inf_select", 1, (5,)), ("log2_left_unscaled", 0, (0, 2, 8))):
        d = R.case(V, variant)
        want = R.reference(d["a"], d["ids"], V, d["target"])
        got = R.reference(d["a"], d["ids"], V, d["target"], fault=fault)
        fails = R.check(got[:4], want, R.bound(d["a"], d["target"]))[0]
        for r in rows:
            assert any(f.startswith(f"row {r}:") for f in fails), (fault, r, fails)


def test_the_inputs_are_what_the_docstring_says():
    for V in R.VS:
        G, W = R.layout(V)
        assert G * W * 256 >= V and (G == 1 or (G - 1) * W * 256 < V) or V == 1000
        v0, v1, v2 = (R.case(V, k) for k in R.VARIANTS)
        s0, s1 = (R.scored_rows(v["ids"], V, v["target"], V) for v in (v0, v1))
        assert (s0 != s1).all() and s0.sum() == 5                             # every kind of row is scored once and skipped once
        for v, s in ((v0, s0), (v1, s1)):
            assert np.isnan(v["a"][~s]).all() and not v["a"].flags.writeable
        assert v1["target"][2] == V and v1["target"][4] == -1 and v1["target"][6] == R.BIG and 0 <= R.BIG % 2 ** 32 < 4
        want0, want1 = (R.reference(v["a"], v["ids"], V, v["target"]) for v in (v0, v1))
        lp, ent, rk, count, _ = want0
        assert rk[0] == 0 and -3 < lp[0] < 0 and rk[6] == 0 and lp[6] == 0 and ent[6] == 0 and np.isfinite(lp[8])
        assert abs(lp[2] + np.log(V)) < 1e-12 and abs(ent[2] - np.log(V)) < 1e-12 and rk[2] == V // 2
        t = v0["target"][4]
        assert (v0["a"][4, [t - 1, t + 1]] == v0["a"][4, t]).all() and rk[4] > 0     # ties below and above the target's column
        lp, ent, rk, count, _ = want1
        assert lp[1] < -90 and lp[5] == -np.inf and np.isfinite(ent[5]) and np.isnan(lp[7]) and np.isnan(ent[7])
        assert (count == s1).all() and (lp[~s1] == 0).all()
        # the index probes: small integers, and every neighbour the layout has moves the target's logit by a whole number
        a, t = v2["a"].astype(np.float64), v2["target"]
        assert v2["ids"] is None and (a == np.round(a)).all() and a.min() == 0 and a.max() == 4 and len(set(t.tolist())) == min(R.M, V)
        for step in (1, 4, 256, W * 256):
            for sign in (-1, 1):
                c = t + sign * step
                ok = (c >= 0) & (c < V)
                assert (np.abs(a[np.arange(R.M), np.where(ok, c, 0)] - a[np.arange(R.M), t])[ok] >= 1).all(), (V, step)


def test_a_flat_row_has_the_entropy_log_v_and_rank_zero_is_the_first_arg_max():
    for V in R.VS:
        x = np.full((1, V), -2.5, np.float32)
        lp, ent, rk = Pipeline._token_logprob_cpu(torch.from_numpy(x), torch.tensor([V - 1]))
        B = R.bound(x, [V - 1], n_adds=V)
        assert abs(float(ent) - np.log(V)) < B[1][0] and abs(float(lp) + np.log(V)) < B[0][0] and int(rk) == V - 1
        rng = np.random.default_rng(V)
        x = np.round(rng.standard_normal((64, V)) * 2).astype(np.float32) / 2            # duplicates of the maximum included
        first = x.argmax(1)                                                              # (numpy: the first of equal maxima)
        for t in (first, np.minimum(first + 1, V - 1), rng.integers(0, V, 64)):
            rk64 = R.values(x, t)[2]
            rk = Pipeline._token_logprob_cpu(torch.from_numpy(x), torch.from_numpy(t))[2].numpy()
            assert (rk == rk64).all() and ((rk == 0) == (t == first)).all()


# ------------------------------------------------------------------------------------------------------------- (b) the pipeline

def combine_cpu(cond, uncond, scale):
    return torch.addcmul(uncond, cond - uncond, torch.tensor(float(scale)))               # the plain-torch branch's expression


def float64_maps(pipe, ids, context, lens, masks, scale, device=None, n_adds=None, combine=combine_cpu):
    """``token_scores``' rule in float64 on the pipeline's OWN logits of the same masked ids -> (means float64 [3, B, N] -- logp, entropy,
    rank --, bounds float64 [2, B, N]).  The bound of a map: the draws' own bounds (tests/logprob_ref.py), one rounding per accumulation
    and one of the division:  (sum_j B_j + draws u sum_j |v_j|) / count + u |mean|."""
    B, N = ids.shape
    V = pipe.mask_token_id
    known = (ids != V).reshape(-1).numpy()
    target = ids.reshape(-1).numpy()
    acc, bsum, asum, count = np.zeros((3, B * N)), np.zeros((2, B * N)), np.zeros((2, B * N)), np.zeros(B * N)
    for m in masks:
        tok = pipe.ids2tokens(torch.where(m, torch.full_like(ids, V), ids).to(device))
        x = pipe.tokens2logits(tok, None if context is None else context.to(device), context_lens=lens)
        if scale is not None:
            x = combine(x, pipe.tokens2logits(tok, None), scale)
        x = x.detach().reshape(B * N, V).cpu().numpy()
        assert x.dtype == np.float32
        vals = R.values(x, target)
        bnd = R.bound(x, target, n_adds=n_adds)
        on = m.reshape(-1).numpy() & known
        acc += np.where(on, np.stack(vals), 0.0)
        bsum += np.where(on, np.stack(bnd), 0.0)
        asum += np.where(on, np.abs(np.stack(vals[:2])), 0.0)
        count += on
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = acc / count
        bound = (bsum + len(masks) * R.U * asum) / count + R.U * np.abs(mean[:2])
    return mean.reshape(3, B, N), bound.reshape(2, B, N)


def check_maps(got, mean, bound, what):
    """got: TokenScores [B, g, g]; the rank's mean exactly (integers), the other two within the bound -> worst err / bound"""
    B = got.logp.shape[0]
    known = ~np.isnan(mean[2])
    rank = got.rank.cpu().reshape(B, -1).numpy()
    assert (np.isnan(rank) == ~known).all() and (rank[known] == mean[2][known].astype(np.float32)).all(), f"{what}: rank"
    worst = 0.0
    for k, name in enumerate(("logp", "entropy")):
        g = getattr(got, name).cpu().reshape(B, -1).double().numpy()
        assert (np.isnan(g) == ~known).all()
        ratio = (np.abs(g - mean[k])[known] / bound[k][known]).max()
        print(f"{what}: {name} worst err / bound {ratio:.4f}")
        assert ratio < 1, (what, name, ratio)
        worst = max(worst, ratio)
    assert (got.logp.cpu().reshape(B, -1).numpy()[known] <= 0).all() and (got.entropy.cpu().reshape(B, -1).numpy()[known] >= 0).all()
    return worst


def score_setting(pipe, device=None):
    """the arguments the two test files score: the photograph (on `device`), its ids (on the CPU), the source context of ``pair_case``
    under its lengths"""
    src, *_ = pair_case(pipe)
    img = photo(pipe).to(device)
    ids = pipe.to_latent(img)[1].reshape(PAIRS, pipe.num_tokens).cpu()
    return img, ids, src, LENS_SRC


@pytest.mark.parametrize("scale", SCALES)
def test_token_scores_is_the_float64_rule_on_the_branchs_own_logits(pipe, scale):
    img, ids, src, lens = score_setting(pipe)
    g, N, V = pipe.image_size // pipe.patch_size, pipe.num_tokens, pipe.mask_token_id
    kw = dict(mask_ratio=0.4, draws=3, seed=7)
    masks = diff_draws(PAIRS, N, 0.4, 3, 7)
    got = pipe.token_scores(img, src, context_lens=lens, guidance_scale=scale, **kw)
    assert isinstance(got, TokenScores) and all(x.dtype == torch.float32 and tuple(x.shape) == (PAIRS, g, g) for x in got)
    check_maps(got, *float64_maps(pipe, ids, src, lens, masks, scale, n_adds=V), f"scale {scale}")
    via_ids = pipe.token_scores(ids=ids.reshape(PAIRS, g, g), text=src, context_lens=lens, guidance_scale=scale, **kw)
    assert all(torch.equal(x, y) for x, y in zip(got, via_ids))
    if scale is None:                                                    # text=None is the unconditional branch
        check_maps(pipe.token_scores(img, None, **kw), *float64_maps(pipe, ids, None, None, masks, None, n_adds=V), "unconditional")
        # a position that holds the mask id is never scored: NaN in the maps, no part of the score
        holes = ids.clone()
        holes[0, 3] = holes[1, 0] = V
        got = pipe.token_scores(ids=holes, text=src, context_lens=lens, **kw)
        mean, bound = float64_maps(pipe, holes, src, lens, masks, None, n_adds=V)
        assert np.isnan(mean[0][0, 3]) and np.isnan(mean[0][1, 0]) and np.isnan(mean[0]).sum() == 2
        check_maps(got, mean, bound, "two mask ids")
        s = pipe.score(ids=holes, text=src, context_lens=lens, **kw)
        want = np.nansum(mean[0], axis=1) / (N - 1)
        assert np.abs(s.double().numpy() - want).max() < np.nansum(bound[0], axis=1).max() / (N - 1) + 2 * N * R.U * np.abs(want).max()


def test_score_surprise_mask_and_the_relative_score(pipe):
    img, ids, src, lens = score_setting(pipe)
    g, N = pipe.image_size // pipe.patch_size, pipe.num_tokens
    kw = dict(context_lens=lens, mask_ratio=0.4, draws=3, seed=7)
    maps = pipe.token_scores(img, src, **kw)
    s = pipe.score(img, src, **kw)
    assert s.dtype == torch.float32 and tuple(s.shape) == (PAIRS,) and torch.equal(s, maps.logp.reshape(PAIRS, N).sum(1) / N) and bool((s <= 0).all())
    un = pipe.score(img, None, mask_ratio=0.4, draws=3, seed=7)
    assert torch.equal(pipe.score(img, src, relative=True, **kw), s - un)
    mask, sur = pipe.surprise_mask(img, src, threshold=0.9, grow=0, return_score=True, **kw)
    assert torch.equal(sur, -maps.logp) and mask.dtype == torch.bool and tuple(mask.shape) == (PAIRS, g, g)
    flat = sur.reshape(PAIRS, N)
    assert torch.equal(mask.reshape(PAIRS, N), Pipeline._region_cpu(flat, flat, g, 0.9, 0)) and 0 < int(mask.sum()) < mask.numel()
    assert torch.equal(pipe.surprise_mask(img, src, threshold=0.9, grow=0, **kw), mask)
    assert torch.equal(pipe.surprise_mask(img, src, **kw).reshape(PAIRS, N), Pipeline._region_cpu(flat, flat, g, 0.5, 1))       # the defaults
    tight = pipe.surprise_mask(img, src, threshold=1.0, grow=0, **kw)
    assert (tight.reshape(PAIRS, N).sum(1) >= 1).all() and torch.equal(tight.reshape(PAIRS, N), flat >= flat.amax(1, keepdim=True))
    # what edit(token_mask=) takes
    out, new = pipe.edit(img, token_mask=mask, text=src, context_lens=lens, timesteps=2, seed=3, return_ids=True)
    outside = ~mask.reshape(PAIRS, N)
    assert torch.equal(new[outside], ids[outside])


def test_best_index():
    nan = float("nan")
    s = torch.tensor([[1.0, 3.0, 3.0, 2.0], [nan, -5.0, nan, -7.0], [nan, nan, nan, nan], [-1.0, nan, -1.0, -2.0], [-np.inf, nan, -np.inf, nan]])
    assert best_index(s).tolist() == [1, 1, 0, 0, 0] and best_index(s).dtype == torch.int64
    assert best_index(torch.tensor([[nan], [2.0]])).tolist() == [0, 0]


def test_best_of(pipe, monkeypatch):
    text = ["a red barn", "the cow"]
    T = 3
    gen = dict(timesteps=T, temperature=0.9, topk=4, seed=11, guidance_scale=1.5)
    imgs, index, scores, cands = pipe.best_of(text, 3, score_draws=2, score_seed=5, image_base=4, return_all=True, **gen)
    N = pipe.num_tokens
    assert tuple(cands.shape) == (2, 3, N) and cands.dtype == torch.int64 and tuple(scores.shape) == (2, 3) and scores.dtype == torch.float32
    assert index.tolist() == best_index(scores).tolist() and imgs.dtype == torch.float32 and tuple(imgs.shape) == (2, 3, pipe.image_size, pipe.image_size)
    ctx = pipe.text_model(text)
    for j in range(3):                                                   # candidate j: the run with image_base + j * B, bit for bit
        run, ids = pipe.generate(text, save_interval=1, image_base=4 + j * 2, return_ids=True, **gen)
        assert torch.equal(ids, cands[:, j])
        assert torch.equal(scores[:, j], pipe.score(ids=ids, text=ctx, draws=2, seed=5))
        for b in range(2):
            if index[b] == j:
                assert torch.equal(imgs[b], run[-1][b])
    one = pipe.best_of(text, 1, **gen)
    assert len(one) == 3 and one[1].tolist() == [0, 0] and torch.equal(one[0], pipe.generate(text, save_interval=1, **gen)[-1])
    # the winner follows injected scores: ties to the lowest j, a NaN never wins
    inject = iter([torch.tensor([-3.0, float("nan")]), torch.tensor([-2.0, -4.0]), torch.tensor([-2.0, -4.0])])
    monkeypatch.setattr(Pipeline, "score", lambda self, **kw: next(inject))
    imgs2, index2, scores2, cands2 = pipe.best_of(text, 3, image_base=4, return_all=True, **gen)
    assert index2.tolist() == [1, 1] and torch.equal(cands2, cands)
    assert torch.isnan(scores2[1, 0]) and scores2[0].tolist() == [-3.0, -2.0, -2.0]


# ------------------------------------------------------------------------------------------------------------- (c) the ABI, the refusals

def test_the_new_symbol_the_header_and_the_prototypes():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "pmhip.h")).read()
    m = re.search(r"int pmhip_token_logprob\(([^;]*)\);", hdr)
    assert m, "pmhip_token_logprob is not declared in include/pmhip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    kinds = ["ptr" if "*" in p else p.split()[0] for p in params[:-1]] + ["ptr"]   # (pmhip_stream is a pointer)
    assert kinds == ["ptr", "ptr", "float", "int", "ptr", "int64_t", "ptr", "ptr", "ptr", "ptr", "ptr", "int", "int", "int", "ptr"]
    as_kind = {C.c_void_p: "ptr", C.c_int: "int", C.c_int64: "int64_t", C.c_float: "float"}
    res, argtypes = _lib.PROTOTYPES["pmhip_token_logprob"]
    assert res is C.c_int and [as_kind[a] for a in argtypes] == kinds
    assert re.search(r"#define PMHIP_ABI_VERSION 11\b", hdr) and _lib.ABI_VERSION == 11
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11 and hasattr(lib, "pmhip_token_logprob")


def test_the_entry_refuses_before_it_launches():
    """every PMHIP_EINVAL of the entry returns in front of the launch: dummy pointers, no GPU"""
    import ctypes as C
    lib = _lib.load()
    p = C.c_void_p(64)

    def rc(a=p, b=None, scale=1.0, ldl=72, ids=p, target=p, logp=p, entropy=p, rank=p, count=p, accumulate=0, M=9, V=64):
        return lib.pmhip_token_logprob(a, b, scale, ldl, ids, 64, target, logp, entropy, rank, count, accumulate, M, V, None)
    for bad, text in ((dict(a=None), b"a is NULL"), (dict(target=None), b"target is NULL"), (dict(logp=None), b"logp is NULL"),
                      (dict(a=C.c_void_p(68)), b"aligned"), (dict(b=C.c_void_p(72)), b"aligned"),
                      (dict(M=0), b"M=0"), (dict(M=-3), b"M=-3"), (dict(V=0), b"V=0"), (dict(V=-4), b"V=-4"), (dict(V=16388, ldl=16388), b"V=16388"),
                      (dict(V=62, ldl=64), b"V=62"), (dict(ldl=70), b"ldl=70"), (dict(ldl=60), b"ldl=60"), (dict(V=1000, ldl=996), b"ldl=996"),
                      (dict(b=p, scale=float("nan")), b"scale=nan"), (dict(b=p, scale=float("inf")), b"scale=inf"),
                      (dict(b=p, scale=float("-inf")), b"scale=-inf")):
        assert rc(**bad) == _lib.PMHIP_EINVAL, bad
        msg = lib.pmhip_last_error()
        assert b"token_logprob" in msg and text in msg, (bad, msg)
        assert not re.search(rb"PMHIP_[A-Z0-9_]+", msg)


def test_the_operators_argument_faults_are_value_errors():
    a, u = torch.zeros(9, 64), torch.zeros(9, 64)
    t = torch.zeros(9, dtype=torch.int64)
    ids = torch.full((9,), 64, dtype=torch.int64)
    wide = torch.zeros(9, 72)
    f, i = torch.zeros(9), torch.zeros(9, dtype=torch.int32)
    for bad in (dict(logits=a.double()), dict(logits=a[0]), dict(logits=None), dict(logits=torch.zeros(9, 62)), dict(logits=torch.zeros(2, 16388), target=t[:2]),
                dict(logits=torch.zeros(0, 64), target=t[:0]), dict(logits=wide[:, 2:66]), dict(logits=a.t().contiguous().t()), dict(logits=torch.zeros(9, 70)[:, :64]),
                dict(target=t.int()), dict(target=t[:8]), dict(target=torch.zeros(18, dtype=torch.int64)[::2]), dict(target=None),
                dict(uncond=u), dict(scale=2.0), dict(uncond=u.half(), scale=2.0), dict(uncond=u[:8], scale=2.0), dict(uncond=wide[:, :64], scale=2.0),
                dict(uncond=u, scale=float("nan")), dict(uncond=u, scale=float("inf")), dict(uncond=u, scale=True), dict(uncond=u, scale="3"),
                dict(ids=ids), dict(mask_id=64), dict(ids=ids, mask_id=64.0), dict(ids=ids, mask_id=True), dict(ids=ids.int(), mask_id=64),
                dict(ids=ids[:8], mask_id=64), dict(accumulate=True)):
        kw = dict(logits=a, target=t)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.token_logprob(**kw)
    with pytest.raises(_lib.PmhipError):                                           # host memory: no CPU fallback
        ops.token_logprob(a, t)
    with pytest.raises(_lib.PmhipError):
        ops.token_logprob(wide[:, :64], t, uncond=torch.zeros(9, 72)[:, :64], scale=3.0, ids=ids, mask_id=64, out=(f, f.clone(), i, i.clone()), accumulate=True)


def test_the_pipeline_calls_argument_faults_are_value_errors(pipe):
    img, ids, src, lens = score_setting(pipe)
    S, V = pipe.image_size, pipe.mask_token_id
    ok = dict(img=img, text=src)
    for bad in (dict(img=None), dict(ids=ids), dict(img=img[0]), dict(img=img[:, :, :S - 8]), dict(img=None, ids=ids.int()), dict(img=None, ids=ids[:, :5]),
                dict(img=None, ids=ids.reshape(-1)), dict(img=None, ids=torch.where(ids == ids[0, 0], V + 1, ids)), dict(img=None, ids=torch.where(ids == ids[0, 0], -1, ids)),
                dict(mask_ratio=0.0), dict(mask_ratio=1.0), dict(draws=0), dict(mask_ratio=0.2, draws=3), dict(seed=0.5),
                dict(guidance_scale=[1.0, 2.0]), dict(guidance_scale=float("nan")), dict(guidance_scale=float("inf")), dict(guidance_scale=True),
                dict(text=None, guidance_scale=2.0), dict(text=None, mask_padding=True), dict(text=None, context_lens=[3, 3]),
                dict(text=src[:1]), dict(text=src[0]), dict(text=["a"]), dict(text=[1, 2]), dict(text=3.0), dict(mask_padding=True), dict(context_lens=[77]),
                dict(context_lens=[77, 0]), dict(negative_text=["x", "y"]), dict(context_segments=np.zeros((2, 77))), dict(token_segments=np.zeros((2, 16))),
                dict(context_weights=np.ones((2, 77))), dict(prompt_weights=True), dict(regions=[])):
        kw = dict(ok)
        kw.update(bad)
        for call in (pipe.token_scores, pipe.score):
            with pytest.raises(ValueError):
                call(**kw)
    for bad in (dict(text=None), dict(guidance_scale=2.0)):
        with pytest.raises(ValueError):
            pipe.score(img, **{**dict(text=src, relative=True), **bad})
    for bad in (dict(threshold=0.0), dict(threshold=1.5), dict(threshold="0.5"), dict(threshold=True), dict(grow=-1), dict(grow=1.0), dict(ids=ids),
                dict(negative_text=["x", "y"]), dict(draws=0)):
        with pytest.raises(ValueError):
            pipe.surprise_mask(img, src, **bad)
    text = ["a", "b"]
    for bad in (dict(n=0), dict(n=True), dict(n=2.0), dict(text="a"), dict(text=[]), dict(text=[1, 2]), dict(image_base=-1), dict(score_guidance=[1.0]),
                dict(score_guidance=float("nan")), dict(score_draws=0), dict(score_mask_ratio=1.0), dict(score_seed=0.5), dict(regions=[[], []]),
                dict(prompt_weights=True), dict(negative_text="x"), dict(context_weights=np.ones((2, 77))), dict(mask=img[:, 0]), dict(token_mask=img[:, 0] > 0),
                dict(top_p=0.0), dict(choice_temperature=-1.0), dict(guidance_scale=[1.0])):
        kw = dict(text=text, n=2, timesteps=2, seed=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            pipe.best_of(**kw)
    assert tuple(pipe.token_scores(img, ["a", "b"]).logp.shape) == (PAIRS, S // pipe.patch_size, S // pipe.patch_size)         # prompts instead of a tensor
