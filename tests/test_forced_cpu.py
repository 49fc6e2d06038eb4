"""The teacher-forced source pass without a GPU.

(a) the bound of tests/forced_ref.py rejects every named fault at exactly the inputs tests/test_gpu_forced.py launches; (b) the
plain-torch step ``Pipeline._forced_cpu`` is the restatement and advances the generator as ``_draw_cpu`` does; (c) the invariants of
``forced_ids`` / ``control_ids(source_ids=)`` / ``prompt_to_prompt(img= / source_ids=)`` on the CPU branch of the tiny pipeline; (d) the
validation; (e) the new symbol, the header, the prototypes and the ABI version; and the conditions on the inputs of the GPU file's
comparison against this branch, met by this branch alone."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import forced_ref as R
from paintmind_amd import _lib
from paintmind_amd.generate import Pipeline, loop_schedule
from paintmind_amd.modules.encoder import T5TextEmbedder
from test_control_cpu import LENS_EDIT, LENS_SRC, PAIRS, CharTokenizer, _tiny, pair_case
from test_local_blend_cpu import phrase_rows
from text_stubs import tiny_t5
from util import ROOT

TOL = 1e-3                                  # the project's float bar (tests/test_gpu_control.py)
SCORE_REL = math.expm1(2 * TOL)             # what it grants a phrase score (tests/test_gpu_local_blend.py)
# the loop the GPU file compares against this branch: chosen here, on the CPU, by the margins test below
LOOP_T, LOOP_TOPK, LOOP_SEED, SOURCE_SEED, NOISE_SEED = 4, 3, 9, 6, 6
LOOP = dict(blend_threshold=0.96, blend_grow=0, blend_start=0.25)
AUDIT_CAP = 0                               # tests/test_gpu_local_blend.py allows its loop no audited position at all (ties == 0)


@pytest.fixture(scope="module")
def pipe():
    return _tiny()


def source_tokens(pipe, seed=SOURCE_SEED):
    """the tokens of 'a real image': seeded codes, int64 [PAIRS, N]"""
    return torch.randint(0, pipe.mask_token_id, (PAIRS, pipe.num_tokens), generator=torch.Generator().manual_seed(seed))


def loop_noise(pipe):
    return torch.rand(LOOP_T, PAIRS, pipe.num_tokens, pipe.mask_token_id, generator=torch.Generator().manual_seed(NOISE_SEED))


# ------------------------------------------------------------------------------------------------------------- (a) the bound

@pytest.mark.parametrize("V", R.VS)
def test_the_bound_rejects_every_named_fault_at_the_gpu_tests_inputs(V):
    rejected = {f: 0 for f in R.FAULTS}
    for variant in (0, 1):
        d = R.case(V, variant)
        want = R.reference(d["logits"], d["ids"], d["target"], V)
        B = R.bound(d["logits"], d["target"])
        assert R.check(want[:3], want[:3], B) == ([], 0.0)
        f32 = (want[0], want[1], want[2].astype(np.float32))                      # the correct answer rounded once: far inside
        fails, worst = R.check(f32, want[:3], B)
        assert not fails and worst < 1.0, (fails, worst)
        for fault in R.FAULTS:
            got = R.reference(d["logits"], d["ids"], d["target"], V, fault)
            rejected[fault] += len(R.check(got[:3], want[:3], B)[0])
    print(f"V={V}: rows on which each fault is rejected: {rejected}")
    assert all(v > 0 for v in rejected.values()), rejected


def test_the_inputs_are_what_the_docstring_says():
    for V in R.VS:
        for variant in (0, 1):
            d = R.case(V, variant)
            x, t, ids = d["logits"], d["target"], d["ids"]
            _, _, score, p = R.reference(x, ids, t, V)
            given = ids != V
            assert int(given.sum()) == (4, 5)[variant] and (ids[given] != t[given]).all() and ((ids >= 0) & (ids <= V)).all()
            assert t[0] == 0 and t[1] == V - 1 and t[2] == int(x[2].argmax()) and t[6] == 0 and t[7] == V - 1
            assert 1e-3 < p[3] < 0.5 and p[4] < 2.0 ** -150 and p[5] == 0.0 and np.isneginf(x[5, t[5]])
            assert np.float32(np.exp(np.float32(x[4, t[4]] - x[4].max()))) == 0.0                  # the class underflows in fp32
            assert (x[6:].max(1) - x[6:].min(1) < 0.5).all()                                       # nearly flat
            last = (R.nv4(V) - 1) * 256
            assert int(x[2].argmax()) >= last and x[2].max() - np.delete(x[2], int(x[2].argmax())).max() > 90
            assert R.M == 2 * R.ROWS_PER_WORKGROUP + 1 and x.shape == (R.M, V) and x.dtype == np.float32
    assert [R.nv4(V) for V in R.VS] == [1, 4, 32, 64] and 1000 % 64 and 1000 % 256


# ------------------------------------------------------------------------------------------------------------- (b) the CPU step

@pytest.mark.parametrize("V", R.VS)
def test_forced_cpu_is_the_restatement(V):
    stub = types.SimpleNamespace(mask_token_id=V)
    for variant in (0, 1):
        d = R.case(V, variant)
        x, ids, t = (torch.from_numpy(np.array(d[k]))[None] for k in ("logits", "ids", "target"))
        pred, merged, score, g = Pipeline._forced_cpu(stub, ids, x, t, None, None)
        assert g is None
        want = R.reference(d["logits"], d["ids"], d["target"], V)
        # torch's fp32 softmax is a chain of its own: the kernel's bound plus 16 roundings of a number at most 1
        fails, worst = R.check((pred[0].numpy(), merged[0].numpy(), score[0].numpy()), want[:3], R.bound(d["logits"], d["target"]) + 16 * R.U)
        assert not fails, fails
        assert score.dtype == torch.float32 and pred.dtype == merged.dtype == torch.int64


def test_forced_cpu_advances_the_generator_as_the_draw_does():
    V = 64
    stub = types.SimpleNamespace(mask_token_id=V)
    d = R.case(V, 0)
    x, ids, t = (torch.from_numpy(np.array(d[k]))[None] for k in ("logits", "ids", "target"))
    x = torch.nan_to_num(x, neginf=-30.0)
    *_, g_draw = Pipeline._draw_cpu(stub, ids, x, 5, 1.0, None, 41)
    *_, g_forced = Pipeline._forced_cpu(stub, ids, x, t, None, 41)
    a, b = torch.rand(7, generator=g_draw), torch.rand(7, generator=g_forced)
    assert torch.equal(a, b)
    fresh = torch.rand(7, generator=torch.Generator().manual_seed(41))
    assert not torch.equal(a, fresh)                                              # (both are BEHIND the token draw's uniforms)
    noise = torch.rand(x.shape, generator=torch.Generator().manual_seed(1))
    *_, g_given = Pipeline._forced_cpu(stub, ids, x, t, noise, 41)
    assert torch.equal(torch.rand(7, generator=g_given), fresh)                   # given noise: nothing is drawn, as in _draw_cpu
    *_, g_draw_given = Pipeline._draw_cpu(stub, ids, x, 5, 1.0, noise, 41)
    assert torch.equal(torch.rand(7, generator=g_draw_given), fresh)


# ------------------------------------------------------------------------------------------------------------- (c) the loops

class Recorder:
    """wraps the halves of the CPU tail of one pipeline: every forced step, draw, blend and re-masking, in call order"""

    def __init__(self, pipe):
        self.pipe, self.forced, self.draws, self.blends, self.remasks, self.after = pipe, [], [], [], [], []
        keep = lambda d: tuple(x.clone() if isinstance(x, torch.Tensor) else x for x in d)
        real = {k: getattr(pipe, k) for k in ("_forced_cpu", "_draw_cpu", "_blend_cpu", "_remask_cpu")}
        pipe._forced_cpu = lambda *a, **kw: (lambda d: (self.forced.append(keep(d)), d)[1])(real["_forced_cpu"](*a, **kw))
        pipe._draw_cpu = lambda *a, **kw: (lambda d: (self.draws.append((keep(a), keep(d))), d)[1])(real["_draw_cpu"](*a, **kw))
        pipe._blend_cpu = lambda *a, **kw: (lambda d: (self.blends.append((a[0].clone(), keep(d))), d)[1])(real["_blend_cpu"](*a, **kw))

        def remask(ids, scores, nm, g, choice_t=0.0, *a, **kw):
            self.remasks.append((ids.clone(), scores.clone(), nm, choice_t))
            out = real["_remask_cpu"](ids, scores, nm, g, choice_t, *a, **kw)
            self.after.append(out.clone())
            return out
        pipe._remask_cpu = remask

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for k in ("_forced_cpu", "_draw_cpu", "_blend_cpu", "_remask_cpu"):
            delattr(self.pipe, k)


def check_source_half(pipe, s, ids_src, T):
    """invariant 3: the source half ends at the real image's tokens, nmask[T - 1] of them still masked"""
    V = pipe.mask_token_id
    nm = loop_schedule(T, 1.0, pipe.num_tokens)[1][T - 1]
    open_ = ids_src != V
    assert torch.equal(ids_src[open_], s.to(ids_src.device)[open_])
    assert ((~open_).sum(1) == nm).all(), ((~open_).sum(1).tolist(), nm)


def check_reveal(pipe, s, per_step, revealed_at, T):
    """invariant 5: revealed_at is the first step after which a position is unmasked, and reveal is monotone -- a revealed position
    stays revealed, at its source token"""
    V = pipe.mask_token_id
    first = torch.full_like(revealed_at, T)
    was = torch.zeros_like(revealed_at, dtype=torch.bool)
    for step, ids in enumerate(per_step):
        now = ids != V
        assert bool((now | ~was).all()), f"step {step}: a revealed position was re-masked"
        assert torch.equal(ids[now], s.to(ids.device)[now])
        first = torch.where(now & (first == T), torch.full_like(first, step), first)
        was = now
    assert torch.equal(first, revealed_at)
    nmask = loop_schedule(T, 1.0, pipe.num_tokens)[1]
    for step in range(T):
        assert ((revealed_at > step).sum(1) == nmask[step]).all()


@pytest.mark.parametrize("ct", [None, 4.0], ids=["plain", "choice"])
@pytest.mark.parametrize("T", [1, 3, 4])
def test_the_invariants_on_the_cpu_branch(pipe, T, ct):
    src, edit, rm, bl, gn = pair_case(pipe)
    N, V, seed = pipe.num_tokens, pipe.mask_token_id, 7
    g = math.isqrt(N)
    s = source_tokens(pipe)
    args = (src, edit, LENS_SRC, LENS_EDIT, rm, bl, gn, PAIRS, T, 1.0, 3, seed)
    kw = dict(cross_steps=0.8, choice_temperature=ct, source_ids=s)
    with Recorder(pipe) as rec:
        alone, revealed = pipe.forced_ids(s, src, PAIRS, T, seed, choice_temperature=ct, context_lens=LENS_SRC, return_steps=True)
    assert len(rec.forced) == T and not rec.draws and torch.equal(pipe.forced_ids(s, src, PAIRS, T, seed, choice_temperature=ct, context_lens=LENS_SRC), alone)
    check_source_half(pipe, s, alone, T)
    check_reveal(pipe, s, rec.after, revealed, T)
    for pred, merged, score, _ in rec.forced:
        assert torch.equal(pred, s) and bool(((score == -1e5) | ((score >= 0) & (score <= 1))).all())
    block = torch.zeros(PAIRS, g, g, dtype=torch.bool)
    block[:, 1:3, 1:3] = True
    ones, zeros = torch.ones_like(block), torch.zeros_like(block)
    plain = pipe.control_ids(*args, **kw)
    assert torch.equal(plain[0], alone)                                           # invariant 2, without a blend
    assert not torch.equal(pipe.control_ids(*args, cross_steps=0.8, choice_temperature=ct)[0], alone)      # (the forced source is another loop)
    for name, blend in (("false", dict(blend_mask=zeros)), ("true", dict(blend_mask=ones)), ("block", dict(blend_mask=block)),
                        ("rows", dict(blend_rows=phrase_rows(), blend_threshold=0.9, blend_grow=0))):
        with Recorder(pipe) as rec:
            ids_s, ids_e, img_s, img_e, mask = pipe.control_ids(*args, **kw, **blend, blend_start=0.0, want_imgs=True, return_mask=True)
        assert torch.equal(ids_s, alone), name                                    # invariant 2: whatever the edited half does
        check_source_half(pipe, s, ids_s, T)
        assert torch.equal(img_s, pipe.vqgan.decode_from_indice(s)), name         # invariant 3: the reconstruction of the input
        assert len(rec.forced) == T and len(rec.draws) == T and len(rec.blends) == T and len(rec.remasks) == 2 * T
        for step in range(T):                                                     # invariant 4
            pred_s, merged_s, score_s, _ = rec.forced[step]
            region, (pred_b, merged_b, score_b) = rec.blends[step]
            (ms, ss, _, _), (me, se, _, _) = rec.remasks[2 * step], rec.remasks[2 * step + 1]
            assert torch.equal(ms, merged_s) and torch.equal(ss, score_s)         # the source half never reads the edited half
            assert torch.equal(me, merged_b) and torch.equal(se, score_b)
            out = ~region
            assert torch.equal(pred_b[out], s[out]) and torch.equal(merged_b[out], merged_s[out]) and torch.equal(score_b[out], score_s[out])
            pred_e, merged_e, score_e = rec.draws[step][1][:3]
            assert torch.equal(pred_b[region], pred_e[region]) and torch.equal(score_b[region], score_e[region])
        out = ~mask.reshape(PAIRS, N)
        assert bool(((ids_e[out] == s[out]) | (ids_e[out] == V)).all()), name
        if name == "false":
            assert torch.equal(ids_e, ids_s) and not mask.any()
        if name == "true":
            assert torch.equal(ids_e, plain[1]) and mask.all()
        if name == "rows":
            assert T == 1 or 0 < int(mask.sum()) < mask.numel()


def test_a_pair_shares_its_remasking_noise_with_a_forced_source(pipe):
    """under a choice temperature the re-masking of both halves draws the same uniforms: the forced step draws and discards the token
    draw's, so the generator it hands on stands where the edited half's stands"""
    src, edit, rm, bl, gn = pair_case(pipe)
    s = source_tokens(pipe)
    seen, real = [], torch.rand
    with Recorder(pipe):
        torch.rand = lambda *a, **kw: (lambda u: (seen.append(u.clone()), u)[1])(real(*a, **kw))
        try:
            pipe.control_ids(src, edit, LENS_SRC, LENS_EDIT, rm, bl, gn, PAIRS, 3, 1.0, 3, 7, choice_temperature=4.0, source_ids=s)
        finally:
            torch.rand = real
    choice = [u for u in seen if tuple(u.shape) == (PAIRS, pipe.num_tokens)]
    assert len(choice) == 2 * 2                                                   # (the last step's choice temperature is 0: no draw)
    assert torch.equal(choice[0], choice[1]) and torch.equal(choice[2], choice[3]) and not torch.equal(choice[0], choice[2])


def test_guidance_composes_with_the_forced_loop(pipe):
    src, edit, rm, bl, gn = pair_case(pipe)
    s = source_tokens(pipe)
    alone = pipe.forced_ids(s, src, PAIRS, 3, 7, guidance_scale=3.0, context_lens=LENS_SRC)
    a, _ = pipe.control_ids(src, edit, LENS_SRC, LENS_EDIT, rm, bl, gn, PAIRS, 3, 1.0, 3, 7, guidance_scale=3.0, source_ids=s)
    assert torch.equal(a, alone)
    check_source_half(pipe, s, alone, 3)
    assert not torch.equal(alone, pipe.forced_ids(s, src, PAIRS, 3, 7, context_lens=LENS_SRC))


def t5_pipe(device=None):
    t5 = _tiny(text_model=T5TextEmbedder(tokenizer=CharTokenizer(), transformer=tiny_t5(), max_length=24))
    return t5 if device is None else t5.to(device)


def test_prompt_to_prompt_from_a_real_image_on_the_cpu():
    t5 = t5_pipe()
    text, edit = ["a red barn", "the cow"], ["a red church", "the big cow"]
    S, N, V = t5.image_size, t5.num_tokens, t5.mask_token_id
    g = S // t5.patch_size
    img = torch.rand(2, 3, S, S, generator=torch.Generator().manual_seed(4)) * 2 - 1
    s = t5.to_latent(img)[1].reshape(2, N)
    kw = dict(mode="replace", timesteps=3, seed=5)
    img_s, img_e = t5.prompt_to_prompt(text, edit, img=img, **kw)
    assert torch.equal(img_s, t5.vqgan.decode_from_indice(s)) and tuple(img_e.shape) == (2, 3, S, S) and torch.isfinite(img_e).all()
    ids_s, ids_e = t5.prompt_to_prompt(text, edit, img=img, return_ids=True, **kw)
    same = t5.prompt_to_prompt(text, edit, source_ids=s, return_ids=True, **kw)
    assert torch.equal(ids_s, same[0]) and torch.equal(ids_e, same[1])
    check_source_half(t5, s, ids_s, 3)
    ctx, lens = t5.text_model(text, return_lens=True)
    assert torch.equal(ids_s, t5.forced_ids(s, ctx, 2, 3, 5, context_lens=lens))
    base = t5.prompt_to_prompt(text, edit, return_ids=True, **kw)
    assert not torch.equal(base[0], ids_s)                                        # without the image: the invented picture of before
    # the local blend on top: outside the region the edited picture keeps the photograph's tokens
    a, b, mask = t5.prompt_to_prompt(text, edit, img=img, local_blend=[("barn", "church"), "cow"], blend_start=0.0, return_ids=True,
                                     return_mask=True, **kw)
    out = ~mask.reshape(2, N)
    assert torch.equal(a, ids_s) and bool(((b[out] == s[out]) | (b[out] == V)).all())
    zeros = torch.zeros(2, g, g, dtype=torch.bool)
    a0, b0 = t5.prompt_to_prompt(text, edit, source_ids=s, blend_mask=zeros, blend_start=0.0, return_ids=True, **kw)
    assert torch.equal(a0, ids_s) and torch.equal(b0, ids_s)
    # (d) the surface's refusals
    for bad in (dict(img=img, source_ids=s), dict(img=img[:1]), dict(source_ids=s[:1]), dict(img=img[:, :, :S - 8]), dict(img=img[0]),
                dict(source_ids=s.int()), dict(source_ids=s[:, :N - 1]), dict(source_ids=s.clone().fill_(V)), dict(source_ids=[[0] * N] * 2),
                dict(img=img, negative_text=["x", "y"]), dict(img=img, guidance_scale=[1.0, 2.0, 3.0])):
        with pytest.raises(ValueError):
            t5.prompt_to_prompt(text, edit, **dict(kw, **bad))


# ------------------------------------------------------------------------------------------------------------- (d) validation

def test_the_source_ids_are_validated_once_at_entry(pipe):
    src, edit, rm, bl, gn = pair_case(pipe)
    N, V = pipe.num_tokens, pipe.mask_token_id
    s = source_tokens(pipe)
    args = (src, edit, LENS_SRC, LENS_EDIT, rm, bl, gn, PAIRS, 2, 1.0, 3, 7)

    def bad_value(v, b=1, i=5):
        x = s.clone()
        x[b, i] = v
        x[1, 9] = v                                                               # a later offender: the message names the first
        return x
    for v in (V, -1, V + 7, 2 ** 40):
        for call in (lambda x: pipe.forced_ids(x, src, PAIRS, 2, 7), lambda x: pipe.control_ids(*args, source_ids=x)):
            with pytest.raises(ValueError, match=rf"image 1, token 5: {v} is no code in \[0, {V}\)"):
                call(bad_value(v))
    for x in (s.int(), s.float(), s[:1], s[:, :N - 1], s.reshape(-1), s.tolist(), None):
        with pytest.raises(ValueError, match="int64"):
            pipe.forced_ids(x, src, PAIRS, 2, 7)
        if x is not None:
            with pytest.raises(ValueError, match="int64"):
                pipe.control_ids(*args, source_ids=x)
    with pytest.raises(ValueError):
        pipe.forced_ids(s, src, PAIRS, 2, 7, guidance_scale=[1.0, 2.0])
    with pytest.raises(ValueError):
        pipe.forced_ids(s, None, PAIRS, 2, 7, guidance_scale=2.0)
    with pytest.raises(ValueError):
        pipe.forced_ids(s, src, PAIRS, 2, 7, choice_temperature=-1.0)
    with pytest.raises(TypeError):
        pipe.forced_ids(s, src, PAIRS, 2, 7, topk=3)                              # nothing is drawn: no sampler keywords
    assert tuple(pipe.forced_ids(s, None, PAIRS, 2, 7).shape) == (PAIRS, N)       # an unconditional loop is served


def test_the_operator_has_no_cpu_fallback():
    from paintmind_amd import ops
    x = torch.zeros(3, 64)
    i = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(_lib.PmhipError):
        ops.sample_rows_forced(x, i, i, 64)


# ------------------------------------------------------------------------------------------------------------- (e) the ABI

def test_the_new_symbol_the_header_and_the_prototypes():
    hdr = open(os.path.join(ROOT, "include", "pmhip.h")).read()
    m = re.search(r"int pmhip_sample_rows_forced\(([^;]*)\);", hdr)
    assert m, "pmhip_sample_rows_forced is not declared in include/pmhip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    kinds = ["ptr" if "*" in p else p.split()[0] for p in params[:-1]] + ["ptr"]  # (pmhip_stream is a pointer)
    assert kinds == ["ptr", "int", "ptr", "ptr", "int64_t", "ptr", "ptr", "ptr", "int", "int", "ptr"]
    import ctypes as C
    as_kind = {C.c_void_p: "ptr", C.c_int: "int", C.c_int64: "int64_t"}
    res, argtypes = _lib.PROTOTYPES["pmhip_sample_rows_forced"]
    assert res is C.c_int and [as_kind[a] for a in argtypes] == kinds
    assert re.search(r"#define PMHIP_ABI_VERSION 11\b", hdr) and _lib.ABI_VERSION == 11
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11 and hasattr(lib, "pmhip_sample_rows_forced")


def test_the_entry_refuses_before_it_launches():
    """every PMHIP_EINVAL of the entry returns in front of the launch: dummy pointers, no GPU"""
    import ctypes as C
    lib = _lib.load()
    p = C.c_void_p(64)

    def rc(logits=p, ldl=72, ids_in=p, target=p, pred=p, ids_out=p, score=p, M=9, V=64):
        return lib.pmhip_sample_rows_forced(logits, ldl, ids_in, target, 64, pred, ids_out, score, M, V, None)
    for bad, text in ((dict(logits=None), b"logits"), (dict(ids_in=None), b"ids_in"), (dict(target=None), b"target"), (dict(ids_out=None), b"ids_out"),
                      (dict(M=0), b"M=0"), (dict(M=-3), b"M=-3"), (dict(V=0), b"V=0"), (dict(V=-4), b"V=-4"), (dict(V=16388, ldl=16388), b"V=16388"),
                      (dict(V=62, ldl=64), b"V=62"), (dict(ldl=70), b"ldl=70"), (dict(ldl=60), b"ldl=60"), (dict(V=1000, ldl=996), b"ldl=996")):
        assert rc(**bad) == _lib.PMHIP_EINVAL, bad
        msg = lib.pmhip_last_error()
        assert b"sample_rows_forced" in msg and text in msg, (bad, msg)
        assert not re.search(rb"PMHIP_[A-Z0-9_]+", msg)


# ------------------------------------------------------------------------------------------------------------- the GPU file's inputs

def loop_margins(pipe, run):
    """run(pipe) under a recorder -> how far the CPU branch's decisions are from flipping, each in units of what the float bar TOL
    grants it: (the smallest top-2 gap of the perturbed logits over the masked positions of every draw, over 2 TOL / temperature -- a
    logit moves by at most TOL; the smallest distance between the last re-masked score and the first kept one, over SCORE_REL times
    the two probabilities -- a logit error of TOL moves a probability by at most expm1(2 TOL) of itself)"""
    with Recorder(pipe) as rec:
        run(pipe)
    gap = math.inf
    for (ids, logits, topk, temperature, noise, *_), _ in rec.draws:
        val, ind = logits.topk(topk, dim=-1)
        z = torch.full_like(logits, float("-inf")).scatter_(2, ind, val) / temperature - torch.log((-torch.log(noise.clamp(min=1e-20))).clamp(min=1e-20))
        top2 = z.topk(2, dim=-1).values
        gap = min(gap, float((top2[..., 0] - top2[..., 1])[ids == pipe.mask_token_id].min()) / (2 * TOL / temperature))
    cut = math.inf
    for _, scores, nm, choice_t in rec.remasks:
        assert not choice_t
        order = scores.sort(dim=-1, descending=True).values
        if nm < order.shape[1]:
            a, b = order[:, nm - 1], order[:, nm]
            assert bool((a >= 0).all())                                           # (the re-masked positions are scored ones)
            moves = SCORE_REL * ((1 - a) + torch.where(b < 0, torch.zeros_like(b), 1 - b))          # a given id's -1e5 does not move
            cut = min(cut, float(((a - b) / moves).min()))
    return gap, cut


def test_the_loops_the_gpu_file_compares_are_far_from_a_tie(pipe):
    """the GPU file holds the fp32 engine to this branch with no audited position (AUDIT_CAP).  Here, on the CPU, the inputs (SOURCE_SEED
    and NOISE_SEED, found by a scan over 8 x 6 seeds on this branch alone) are shown to keep every decision of both loops further from
    flipping than the float bar can move it: every top-2 gap, every re-masking cut (loop_margins) and every phrase score against
    threshold * max (SCORE_REL of both sides, as tests/test_gpu_local_blend.py has it).  Two runs of this branch agree exactly."""
    src, edit, rm, bl, gn = pair_case(pipe)
    s, noise, rows = source_tokens(pipe), loop_noise(pipe), phrase_rows()
    args = (src, edit, LENS_SRC, LENS_EDIT, rm, bl, gn, PAIRS, LOOP_T, 1.0, LOOP_TOPK, LOOP_SEED)
    forced = lambda p: p.forced_ids(s, src, PAIRS, LOOP_T, LOOP_SEED, context_lens=LENS_SRC)
    seen, real = [], pipe._region_cpu
    pipe._region_cpu = lambda a, b, *r, **kw: (seen.append((a.double().numpy(), b.double().numpy())), real(a, b, *r, **kw))[1]
    control = lambda p: p.control_ids(*args, cross_steps=0.75, noise=noise, blend_rows=rows, source_ids=s, return_mask=True, **LOOP)
    try:
        gap, cut = loop_margins(pipe, control)
    finally:
        del pipe._region_cpu
    _, cut_alone = loop_margins(pipe, forced)
    t_ = LOOP["blend_threshold"]
    closest = min(float((np.abs(x - t_ * x.max(1, keepdims=True)) / (SCORE_REL * (x + t_ * x.max(1, keepdims=True)))).min())
                  for halves in seen for x in halves)
    print(f"in units of what the float bar grants: top-2 gap {gap:.2f}, re-masking cut {min(cut, cut_alone):.2f}, phrase score {closest:.2f}")
    assert len(seen) == LOOP_T - math.ceil(LOOP["blend_start"] * LOOP_T)
    assert gap > 1.0 and min(cut, cut_alone) > 1.0 and closest > 1.0, "a decision lies within the float bar: choose other seeds"
    one, two = control(pipe), control(pipe)
    differing = sum(int((a != b).sum()) for a, b in zip(one, two)) + int((forced(pipe) != forced(pipe)).sum())
    assert differing <= AUDIT_CAP
    assert 0 < int(one[2].sum()) < one[2].numel()                                 # (the region decides something)
