"""Cross-attention control on the CPU: the bound of tests/control_ref.py against the float32 restatement of the
kernels' arithmetic, at the very inputs tests/test_gpu_attention_control.py runs -- the correct restatement stays below a stated
fraction of the bound, every named fault exceeds it -- and the exact family's expectation; then prompt.align_rows on hand-written
cases."""
import numpy as np
import pytest

import attention_probes as P
import control_ref as C
from paintmind_amd.prompt import align_rows                 # (new with this feature: without it nothing in this file runs)

SIGMAS = (2.0, 8.0)
DHS = (64, 32)
# measured here, on the CPU, over every case below (the figures are in DESIGN.md 4za): the f32 restatement reaches 0.0033 of the
# bound; with P rounded to bf16 0.956, with a bf16 output 0.965, with both 0.939 -- a correctly rounded value can err by almost
# the whole unit roundoff the bound grants, so those three stay below 1 and not far below
FRACTION_F32 = 0.01
FRACTION_ROUNDED = 1.0


def cases():
    for dh in DHS:
        for exp2 in (True, False):
            for Ls, Lt in C.SHAPES:
                for kind in C.LENS:
                    for sigma in SIGMAS:
                        yield dh, exp2, Ls, Lt, kind, sigma


@pytest.fixture(scope="module")
def refs():
    """every case with its float64 reference: computed once, shared, never modified"""
    out = {}
    for key in cases():
        dh, exp2, Ls, Lt, kind, sigma = key
        d = C.case(Ls, Lt, dh, sigma, kind)
        out[key] = (d, C.reference(d, exp2))
    return out


def test_the_restatement_stays_below_a_fraction_of_the_bound(refs):
    worst = {}
    for key, (d, r) in refs.items():
        exp2 = key[1]
        for round_p in (False, True):
            for bf16_out in (False, True):
                e = C.emulate(d, exp2, round_p=round_p)
                ratio, idx = C.worst(P.bf16_round(e) if bf16_out else e, r["ref"], C.bound(d, r, exp2, round_p, bf16_out))
                worst[round_p, bf16_out] = max(worst.get((round_p, bf16_out), 0.0), ratio)
                assert ratio < (FRACTION_ROUNDED if round_p or bf16_out else FRACTION_F32), (key, round_p, bf16_out, idx, ratio)
    print("largest err / bound of the restatement by (P rounded, bf16 output):", {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("fault", C.FAULTS)
def test_every_named_fault_exceeds_the_bound(refs, fault):
    """against the LOOSEST bound (P rounded, bf16 output), in every case where the fault changes the arithmetic at all"""
    least, n = np.inf, 0
    for key, (d, r) in refs.items():
        if not C.fault_applies(fault, d):
            continue
        exp2 = key[1]
        out = P.bf16_round(C.emulate(d, exp2, round_p=True, fault=fault))
        ratio, idx = C.worst(out, r["ref"], C.bound(d, r, exp2, True, True))
        assert ratio > 1.0, (fault, key, idx, ratio)
        least, n = min(least, ratio), n + 1
    print(f"{fault}: {n} cases, exceeds the bound by a factor of at least {least:.3g}")
    assert n >= 48, (fault, n)


def test_the_exact_family_is_exact():
    """the expectation is the same in both units, a multiple of 1/4 below 32 -- representable in bf16 --, and the restatement meets it
    bit for bit with and without the rounding of P"""
    for Ls, Lt in C.SHAPES:
        for kind in C.LENS:
            for dh in DHS:
                d = C.exact_case(Ls, Lt, dh, kind)
                expect = C.reference(d, True)["ref"]
                assert np.array_equal(expect, C.reference(d, False)["ref"])
                assert np.array_equal(expect * 4, np.round(expect * 4)) and np.abs(expect).max() < 32 and P.is_bf16(expect.astype(np.float32))
                for exp2 in (True, False):
                    for round_p in (False, True):
                        assert np.array_equal(C.emulate(d, exp2, round_p=round_p), expect), (Ls, Lt, kind, dh, exp2, round_p)
                if Lt > 1:
                    assert np.abs(expect).max() > 0


def test_poison_marks_exactly_what_may_reach_nothing():
    d = C.case(77, 129, 32, 2.0, "one_mid")
    ksp, ktp, vtp = C.poison(d)
    ns, nt = C.clamp(d["lens_s"], 2, 77), C.clamp(d["lens_t"], 2, 129)
    for b in range(2):
        assert np.isfinite(ksp[b, :, :ns[b]]).all() and np.isnan(ksp[b, :, ns[b]:]).all()
        assert np.isfinite(ktp[b, :, :nt[b]]).all() and np.isnan(ktp[b, :, nt[b]:]).all()
        assert np.isfinite(vtp[b, :, :, :nt[b]]).all() and np.isnan(vtp[b, :, :, nt[b]:]).all()
    assert ksp.shape[2] == 128 and ktp.shape[2] == 192 and vtp.shape[3] == 192
    rm = d["row_map"]
    assert (rm == -1).any() and (rm >= ns[:, None]).any() and (rm[:, 0] == rm[:, 1]).all()


# ------------------------------------------------------------------------------------------------------------- align_rows

def test_align_rows_on_hand_written_cases():
    E = 1                                                     # the end-of-sequence id
    same = [5, 6, 7, E]
    assert align_rows(same, same) == ([0, 1, 2, 3], [1.0, 1.0, 1.0, 1.0])
    assert align_rows(same, same, mode="replace") == ([0, 1, 2, 3], [1.0, 1.0, 1.0, 1.0])
    # one word swapped, equal token counts: 7 -> 9
    src, tgt = [5, 6, 7, 8, E], [5, 6, 9, 8, E]
    assert align_rows(src, tgt) == ([0, 1, -1, 3, 4], [1.0, 1.0, 0.0, 1.0, 1.0])
    assert align_rows(src, tgt, mode="replace") == ([0, 1, 2, 3, 4], [1.0, 1.0, 1.0, 1.0, 1.0])
    # one word swapped, unequal token counts: one source row (7) for three target rows, and two source rows for three
    assert align_rows([5, 7, 8, E], [5, 9, 10, 11, 8, E], mode="replace") == ([0, 1, 1, 1, 2, 3], [1.0] * 6)
    assert align_rows([5, 7, 12, 8, E], [5, 9, 10, 11, 8, E], mode="replace") == ([0, 1, 1, 2, 3, 4], [1.0] * 6)      # floor(i * 2 / 3)
    assert align_rows([5, 9, 10, 11, 8, E], [5, 7, 8, E], mode="replace") == ([0, 1, 4, 5], [1.0] * 4)                # floor(0 * 3 / 1)
    assert align_rows([5, 7, 8, E], [5, 9, 10, 11, 8, E]) == ([0, -1, -1, -1, 2, 3], [1.0, 0.0, 0.0, 0.0, 1.0, 1.0])
    # words inserted: nothing between the same anchors in the source (m = 0), so replace behaves as refine
    for mode in ("refine", "replace"):
        assert align_rows([5, 8, E], [5, 6, 7, 8, E], mode=mode) == ([0, -1, -1, 1, 2], [1.0, 0.0, 0.0, 1.0, 1.0])
        # words removed: every target row has its pair
        assert align_rows([5, 6, 7, 8, E], [5, 8, E], mode=mode) == ([0, 3, 4], [1.0, 1.0, 1.0])
    # empty overlap: only the end-of-sequence rows pair
    assert align_rows([5, 6, E], [7, 8, 9, E]) == ([-1, -1, -1, 2], [0.0, 0.0, 0.0, 1.0])
    assert align_rows([5, 6, E], [7, 8, 9, E], mode="replace") == ([0, 0, 1, 2], [1.0, 1.0, 1.0, 1.0])
    # ties go to the earliest source row: the target's 6 pairs with the first 6
    assert align_rows([6, 6, E], [6, E]) == ([0, 2], [1.0, 1.0])
    assert align_rows([5, 6, 5, 6, E], [5, 6, E]) == ([0, 1, 4], [1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        align_rows(same, same, mode="swap")
    with pytest.raises(ValueError):
        align_rows([], same)


# ------------------------------------------------------------------------------------------------------------- the CPU branch

import torch                                                                     # noqa: E402

import paintmind_amd as pm                                                       # noqa: E402
from paintmind_amd.generate import Pipeline                                      # noqa: E402
from paintmind_amd.modules.encoder import CLIPTextEmbedder, SyntheticTextEmbedder, T5TextEmbedder     # noqa: E402
from text_stubs import StubClipTextTower, stub_clip_tokenize, tiny_t5            # noqa: E402
from util import load_golden, to_torch_sd                                        # noqa: E402

PAIRS, LENS_SRC, LENS_EDIT = 2, [77, 50], [60, 33]


def _tiny(text_model=None):
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False, text_model=text_model)
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.eval()


@pytest.fixture(scope="module")
def pipe():
    return _tiny()


def pair_case(pipe):
    """two pairs, lengths 77 / 50 and 60 / 33, NaN in every context row behind its length; a map with repeats, -1 and entries at or
    behind the source length, blends in {0, 0.3, 0.5, 1}, gains in {0, 0.5, 1, 1.7, 2}"""
    rows = pipe.text_model(["a", "b", "c", "d"]).cpu()
    for b, n in enumerate(LENS_SRC + LENS_EDIT):
        rows[b, n:] = float("nan")
    rm, bl, gn = C.controls(PAIRS, 77, 77, seed=3)
    rm = np.where(rm >= 77, 76, rm)                            # (the model level refuses entries at or above L; 76 is behind pair 1's 50)
    return rows[:PAIRS].contiguous(), rows[PAIRS:].contiguous(), rm, bl, gn


def test_the_cpu_branch_is_the_formula_from_each_controlled_layers_input(pipe):
    """an independent float64 restatement of the controlled cross-attention from the layer's own input (seen by wrapping attn2.run per
    instance) and its weights; the source half is the uncontrolled call bit for bit; self-attention injection likewise"""
    src, edit, rm, bl, gn = pair_case(pipe)
    ctx, lens = torch.cat([src, edit]), LENS_SRC + LENS_EDIT
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, pipe.mask_token_id, (2 * PAIRS, pipe.num_tokens), generator=g)
    ids[torch.rand(2 * PAIRS, pipe.num_tokens, generator=g) < 0.5] = pipe.mask_token_id
    tok = pipe.ids2tokens(ids)
    tr = pipe.transformer
    seen = {}

    def tap(name, attn):
        run = attn.run
        def wrapped(x, context=None, residual=None, **kw):
            out = run(x, context, residual=residual, **kw)
            seen[name] = (x.detach().clone(), None if context is None else context.detach().clone(), residual.detach().clone(), dict(kw), out.detach().clone())
            return out
        attn.run = wrapped
        return run

    layer = tr.layers[1]
    saved = [(layer.attn1, tap("self", layer.attn1)), (layer.attn2, tap("cross", layer.attn2))]
    try:
        with torch.no_grad():
            plain = tr(tok, ctx, context_lens=lens)
            got = tr(tok, ctx, context_lens=lens, control=dict(row_map=rm, blend=bl, gain=gn, cross_layers=[1], self_layers=[1]))
    finally:
        for attn, run in saved:
            del attn.run
    assert torch.isfinite(got).all() and float((got[PAIRS:] - plain[PAIRS:]).abs().max()) > 1e-3
    f8 = lambda t: t.double().numpy()

    def heads(attn, x, w):
        y = f8(x) @ f8(w.detach()).T
        return y.reshape(y.shape[0], y.shape[1], attn.heads, attn.dim_head).transpose(0, 2, 1, 3)

    def softmax(s):
        e = np.exp(s - s.max(-1, keepdims=True))
        return e / e.sum(-1, keepdims=True)

    # the cross-attention of layer 1
    x, c, res, kw, out = seen["cross"]
    a = layer.attn2
    assert kw.get("control") is not None and kw["context_lens"] == lens
    c0 = torch.nan_to_num(c)
    q, k, v = heads(a, x, a.to_q.weight) * a.scale, heads(a, c0, a.to_k.weight), heads(a, c0, a.to_v.weight)
    live = np.arange(77)[None, :] < np.asarray(lens)[:, None]
    p = softmax(np.where(live[:, None, None, :], q @ k.transpose(0, 1, 3, 2), -np.inf))
    v = np.where(live[:, None, :, None], v, 0.0)
    P = p.copy()
    for b in range(PAIRS):
        for j in range(LENS_EDIT[b]):
            m, w = int(rm[b, j]), float(bl[b, j])
            pj = p[PAIRS + b, :, :, j]
            if 0 <= m < LENS_SRC[b] and w != 0:
                pj = (1 - w) * pj + w * p[b, :, :, m]
            P[PAIRS + b, :, :, j] = float(gn[b, j]) * pj
    o = (P @ v).transpose(0, 2, 1, 3).reshape(x.shape[0], x.shape[1], -1)
    want = o @ f8(a.to_out[0].weight.detach()).T + f8(a.to_out[0].bias.detach()) + f8(res)
    err = float(np.abs(f8(out) - want).max())
    print(f"controlled cross-attention, CPU branch against the float64 restatement: {err:.3e}")
    assert err < 1e-4
    # the self-attention of layer 1: the edited half on the source half's q and k
    x, _, res, kw, out = seen["self"]
    a = layer.attn1
    assert kw.get("inject_self") is True
    q, k, v = heads(a, x, a.to_q.weight) * a.scale, heads(a, x, a.to_k.weight), heads(a, x, a.to_v.weight)
    q[PAIRS:], k[PAIRS:] = q[:PAIRS], k[:PAIRS]
    o = (softmax(q @ k.transpose(0, 1, 3, 2)) @ v).transpose(0, 2, 1, 3).reshape(x.shape[0], x.shape[1], -1)
    want = o @ f8(a.to_out[0].weight.detach()).T + f8(a.to_out[0].bias.detach()) + f8(res)
    err = float(np.abs(f8(out) - want).max())
    print(f"injected self-attention, CPU branch against the float64 restatement: {err:.3e}")
    assert err < 1e-4
    assert torch.equal(got[:PAIRS], plain[:PAIRS])                                # the source half never sees the control
    with torch.no_grad():                                                        # blend 0 and gain 1: the call without control
        same = tr(tok, ctx, context_lens=lens, control=dict(row_map=rm, blend=np.zeros_like(bl), gain=np.ones_like(gn), cross_layers=[0, 1]))
    assert float((same - plain).abs().max()) < 1e-5
    for bad in (dict(cross_layers=[0]), dict(row_map=rm, blend=bl, gain=gn), dict(row_map=rm, blend=bl, gain=gn, cross_layers=[2]),
                dict(row_map=rm, blend=bl + 1, gain=gn, cross_layers=[0]), dict(row_map=rm, blend=bl, gain=-gn - 1, cross_layers=[0]),
                dict(row_map=np.full_like(rm, 77), blend=bl, gain=gn, cross_layers=[0]), dict(row_map=rm, blend=bl, gain=gn, self_layers=[0])):
        with pytest.raises(ValueError):
            tr(tok, ctx, context_lens=lens, control=bad)


def test_control_ids_on_the_cpu(pipe):
    """ids_src is the plain loop on the source alone; without controlled steps ids_edit is the plain loop on the edited context; with
    them it differs; guidance composes; a pair shares its noise"""
    src, edit, rm, bl, gn = pair_case(pipe)
    T, seed = 4, 7
    plain = lambda c, n, **kw: pipe._generate_cpu(c, PAIRS, T, 1.0, pipe._options(3, None, kw.get("g"), n, None, c, PAIRS), 1, seed, True)[1]
    a, b = pipe.control_ids(src, edit, LENS_SRC, LENS_EDIT, rm, bl, gn, PAIRS, T, 1.0, 3, seed, cross_steps=0.8, self_steps=0.5)
    assert torch.equal(a, plain(src, LENS_SRC))
    a0, b0 = pipe.control_ids(src, edit, LENS_SRC, LENS_EDIT, rm, bl, gn, PAIRS, T, 1.0, 3, seed, cross_steps=0, self_steps=0)
    assert torch.equal(a0, a) and torch.equal(b0, plain(edit, LENS_EDIT))
    assert not torch.equal(b, b0) and tuple(b.shape) == (PAIRS, pipe.num_tokens)
    ag, bg = pipe.control_ids(src, edit, LENS_SRC, LENS_EDIT, rm, bl, gn, PAIRS, T, 1.0, 3, seed, guidance_scale=3.0, cross_steps=0, self_steps=0)
    assert torch.equal(ag, plain(src, LENS_SRC, g=3.0)) and torch.equal(bg, plain(edit, LENS_EDIT, g=3.0))
    same_a, same_b = pipe.control_ids(src, src, LENS_SRC, LENS_SRC, rm, np.zeros_like(bl), np.ones_like(gn), PAIRS, T, 1.0, 3, seed)
    assert torch.equal(same_a, same_b)                                           # one prompt twice, no control: one image twice
    for bad in (dict(cross_steps=1.5), dict(layers=[2]), dict(layers=[]), dict(guidance_scale=[1.0] * T)):
        with pytest.raises(ValueError):
            pipe.control_ids(src, edit, LENS_SRC, LENS_EDIT, rm, bl, gn, PAIRS, T, 1.0, 3, seed, **bad)
    with pytest.raises(ValueError):
        pipe.control_ids(src, edit[:1], LENS_SRC, LENS_EDIT, rm, bl, gn, PAIRS, T, 1.0, 3, seed)
    with pytest.raises(ValueError):
        pipe.control_ids(src, edit, LENS_SRC, None, rm, bl, gn, PAIRS, T, 1.0, 3, seed)


class CharTokenizer:
    """one id per character (2 + ord % 100), pad 0, end-of-sequence 1; both call forms the embedder uses"""
    pad_token_id, eos_token_id = 0, 1

    @staticmethod
    def ids_of(s):
        return [2 + ord(c) % 100 for c in s]

    def __call__(self, text, max_length=77, add_special_tokens=True, **kw):
        if isinstance(text, str):
            return {"input_ids": self.ids_of(text) + ([1] if add_special_tokens else [])}
        out = torch.zeros(len(text), max_length, dtype=torch.long)
        for i, s in enumerate(text):
            row = self.ids_of(s)[:max_length - 1] + [1]
            out[i, :len(row)] = torch.tensor(row)
        return {"input_ids": out}


def test_fragment_ids_agree_with_phrase_rows_and_the_other_embedders_refuse():
    emb = T5TextEmbedder(tokenizer=CharTokenizer(), transformer=tiny_t5(), max_length=24)
    calls = []
    tower_forward = emb.transformer.forward
    emb.transformer.forward = lambda *a, **kw: (calls.append(kw["input_ids"].clone()), tower_forward(*a, **kw))[1]
    context, lens, ids, spans = emb.fragment_ids([["a ", "red barn", " here"], ["barn"], ["the ", "barn", "z" * 40]])
    assert len(calls) == 1                                                       # ONE tower call, the ids beside it
    assert lens.tolist() == [16, 5, 24] and [len(r) for r in ids] == [16, 5, 24]
    assert ids[0] == CharTokenizer.ids_of("a red barn here") + [1] and ids[2][-1] == 1
    assert spans[0] == [(0, 2), (2, 10), (10, 15)] and spans[1] == [(0, 4)] and spans[2] == [(0, 4), (4, 8), (8, 23)]
    ctx_p, lens_p, rows = emb.phrase_rows(["a red barn here", "barn", "the barn" + "z" * 40], ["red barn", "barn", "barn"])
    assert torch.equal(context, ctx_p) and torch.equal(lens, lens_p)
    for b, (lo, hi) in enumerate((spans[0][1], spans[1][0], spans[2][1])):
        assert rows[b].nonzero().flatten().tolist() == list(range(lo, hi))
    with pytest.raises(NotImplementedError, match="token ids"):
        SyntheticTextEmbedder(96).fragment_ids([["a"]])
    with pytest.raises(NotImplementedError, match="token ids"):
        CLIPTextEmbedder(model=StubClipTextTower(), tokenizer=stub_clip_tokenize).fragment_ids([["a"]])


def test_prompt_to_prompt_end_to_end_on_the_cpu(pipe):
    t5 = _tiny(text_model=T5TextEmbedder(tokenizer=CharTokenizer(), transformer=tiny_t5(), max_length=24))
    calls = []
    control_ids = t5.control_ids
    t5.control_ids = lambda *a, **kw: (calls.append(a), control_ids(*a, **kw))[1]
    text, edit = ["a red barn", "the cow"], ["a red church", "the big cow"]
    img_s, img_e = t5.prompt_to_prompt(text, edit, mode="replace", reweight={"church": 2.0, "big": 0.5}, timesteps=3, seed=5)
    S = t5.image_size
    assert tuple(img_s.shape) == tuple(img_e.shape) == (2, 3, S, S) and torch.isfinite(img_e).all()
    src, tgt, lens_s, lens_e, rm, bl, gn = calls[0][:7]
    assert lens_s == [11, 8] and lens_e == [13, 12]                              # always under the non-pad lengths
    # per character: "a red " pairs, then the r of barn with the r of church; "chu" lies over "ba", "ch" over "n"
    assert rm[0, :13].tolist() == [0, 1, 2, 3, 4, 5, 6, 6, 7, 8, 9, 9, 10] and (rm[0, 13:] == -1).all() and (bl[0, :13] == 1).all()
    assert gn[0].tolist() == [1.0] * 6 + [2.0] * 6 + [1.0] * 12                  # the gain sits on the phrase's rows
    assert rm[1, :12].tolist() == [0, 1, 2, 3, -1, -1, -1, -1, 4, 5, 6, 7] and bl[1, :12].tolist() == [1.0] * 4 + [0.0] * 4 + [1.0] * 4
    assert gn[1].tolist() == [1.0] * 4 + [0.5] * 3 + [1.0] * 17
    ids_s, ids_e = t5.prompt_to_prompt(text, edit, mode="replace", reweight={"church": 2.0, "big": 0.5}, timesteps=3, seed=5, return_ids=True)
    assert not torch.equal(ids_s, ids_e) and tuple(ids_e.shape) == (2, t5.num_tokens)
    ctx, lens = t5.text_model(text, return_lens=True)
    opts = t5._options(5, None, None, lens, None, ctx, 2)
    plain_imgs, plain_ids = t5._generate_cpu(ctx, 2, 3, 1.0, opts, 1, 5, True)
    assert torch.equal(ids_s, plain_ids) and torch.equal(img_s, plain_imgs[-1])                              # the source is the plain image
    # pure re-weighting: one prompt twice, a gain on one word
    r_s, r_e = t5.prompt_to_prompt("a red barn", "a red barn", reweight={"red": 4.0}, timesteps=3, seed=5, return_ids=True)
    assert calls[-1][4].tolist()[0][:11] == list(range(11)) and calls[-1][6][0, 2:5].tolist() == [4.0] * 3 and r_s.shape == (1, t5.num_tokens)
    for bad, kind in ((dict(negative_text=["x", "y"]), ValueError), (dict(regions=[]), ValueError), (dict(prompt_weights=True), ValueError),
                      (dict(context_weights=np.ones((2, 24))), ValueError), (dict(context_segments=np.zeros((2, 24))), ValueError),
                      (dict(guidance_scale=[1.0, 2.0, 3.0]), ValueError), (dict(reweight={"zebra": 2.0}), ValueError),
                      (dict(reweight={"cow": -1.0}), ValueError), (dict(mode="swap"), ValueError)):
        with pytest.raises(kind):
            t5.prompt_to_prompt(text, edit, timesteps=3, seed=5, **bad)
    with pytest.raises(NotImplementedError, match="token ids"):
        pipe.prompt_to_prompt(["a"], ["b"], timesteps=2, seed=1)                 # the synthetic embedder has no tokenizer
    with pytest.raises(ValueError, match="text condition"):
        t5.prompt_to_prompt(None, edit, timesteps=2, seed=1)
