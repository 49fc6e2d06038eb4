"""Cross-attention maps on the plain-torch branch, no GPU: ``Pipeline.attention_maps`` against an independent
float64 restatement computed from each chosen layer's INPUT (seen by wrapping ``attn2._run_cpu`` per instance) and its to_q / to_k
weights, in every form and for several layer subsets; ``tokens2logits`` unchanged bit for bit; ``T5TextEmbedder.phrase_rows`` with
an injected character tokenizer; ``phrase_mask`` against a numpy restatement of its rule; ``edit`` under a phrase mask."""
import numpy as np
import pytest
import torch

import paintmind_amd as pm
import region_ref as R
from paintmind_amd.generate import Pipeline
from paintmind_amd.modules.encoder import CLIPTextEmbedder, SyntheticTextEmbedder, T5TextEmbedder
from text_stubs import StubClipTextTower, stub_clip_tokenize, tiny_t5
from util import load_golden, to_torch_sd

B = 3
FORMS = ("plain", "lens", "regions", "weights", "weights+regions")
LAYER_SETS = (None, [0], [1], [1, 0])


def _tiny(text_model=None):
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False, text_model=text_model)
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.eval()


@pytest.fixture(scope="module")
def pipe():
    return _tiny()


@pytest.fixture(scope="module")
def ids(pipe):
    g = torch.Generator().manual_seed(11)
    out = torch.randint(0, pipe.mask_token_id, (B, pipe.num_tokens), generator=g)
    out[torch.rand(B, pipe.num_tokens, generator=g) < 0.5] = pipe.mask_token_id
    return out


def case(pipe, form):
    """-> (context with NaN in the rows that may reach nothing, keywords, allowed bool [B, N, L], w float64 [B, L])"""
    rows = pipe.text_model(["a", "b", "c", "d", "e", "f"]).cpu()
    L, N = 77, pipe.num_tokens
    context, kw = rows[:B].clone(), {}
    ks = np.zeros((B, L), np.uint8)
    qm = np.full((B, N), 0xFFFFFFFF, np.uint32)
    if form in ("lens", "weights"):
        lens = [77, 50, 33]
        kw["context_lens"] = lens
        ks = np.where(np.arange(L)[None, :] < np.asarray(lens)[:, None], 0, R.PAD).astype(np.uint8)
    if form in ("regions", "weights+regions"):
        S, g = pipe.image_size, pipe.image_size // pipe.patch_size
        left = torch.zeros(S, S)
        left[:, :S // 2] = 1
        tm = torch.zeros(g, g, dtype=torch.bool)
        tm[1:3, 1:3] = True
        regions = [[(rows[3, :40], left), (rows[4, :9], tm)], [(rows[5, :25], tm)], []]
        context, ks, qm = R.layout([rows[b] for b in range(B)], regions, pipe.image_size, pipe.patch_size)
        kw.update(context_segments=ks, token_segments=qm)
    w = np.ones(ks.shape, np.float32)
    if form.startswith("weights"):
        w = np.random.default_rng(1).choice(np.array([0, 0.125, 1, 8, 1.3, 0.5], np.float32), size=ks.shape).astype(np.float32)
        for b in range(B):
            for sg in np.unique(ks[b][ks[b] < 32]):
                w[b, np.flatnonzero(ks[b] == sg)[0]] = (8, 0.125, 1.3)[int(sg) % 3]
        kw["context_weights"] = w
    ksl = ks.astype(np.int64)[:, None, :]
    ok = (ksl < 32) & (((qm.astype(np.int64)[:, :, None] >> np.minimum(ksl, 31)) & 1) == 1) & (w > 0)[:, None, :]
    context = context.clone()
    context[torch.from_numpy(~ok.any(1))] = float("nan")
    return context, kw, ok, w.astype(np.float64)


def restate(attn, x, ctx, ok, w):
    """one layer's head-mean cross-attention probabilities in float64, from the layer's input and its to_q / to_k weights alone"""
    f = lambda t: t.detach().double().numpy()
    h, d = attn.heads, attn.dim_head
    Bx, N, _ = x.shape
    c = np.nan_to_num(f(ctx))
    q = (f(x) @ f(attn.to_q.weight).T * d ** -0.5).reshape(Bx, N, h, d).transpose(0, 2, 1, 3)
    k = (c @ f(attn.to_k.weight).T).reshape(Bx, c.shape[1], h, d).transpose(0, 2, 1, 3)
    out = np.zeros((Bx, N, c.shape[1]))
    for b in range(Bx):
        for hh in range(h):
            for i in range(N):
                js = np.flatnonzero(ok[b, i])
                s = k[b, hh, js] @ q[b, hh, i]
                e = w[b, js] * np.exp(s - s.max())
                out[b, i, js] += e / e.sum() / h
    return out


@pytest.mark.parametrize("form", FORMS)
def test_attention_maps_against_the_float64_restatement(pipe, ids, form):
    context, kw, ok, w = case(pipe, form)
    seen = {}
    try:
        for i, layer in enumerate(pipe.transformer.layers):
            def spy(x, ctx, *a, _i=i, _orig=layer.attn2._run_cpu, **k):
                seen[_i] = (x.clone(), ctx.clone())
                return _orig(x, ctx, *a, **k)
            layer.attn2._run_cpu = spy
        plain = pipe.tokens2logits(pipe.ids2tokens(ids), context, **kw)
        g = pipe.image_size // pipe.patch_size
        for layers in LAYER_SETS:
            seen.clear()
            maps, logits = pipe.attention_maps(ids, context, layers=layers, return_logits=True, **kw)
            assert torch.equal(logits, plain)                                     # unchanged bit for bit when maps are requested
            L = context.shape[1]
            assert maps.shape == (B, L, g, g) and maps.dtype == torch.float32 and torch.isfinite(maps).all()
            chosen = list(range(len(pipe.transformer.layers))) if layers is None else layers
            want = sum(restate(pipe.transformer.layers[l].attn2, *seen[l], ok, w) for l in chosen) / len(chosen)
            got = maps.reshape(B, L, -1).transpose(1, 2).double().numpy()
            err = np.abs(got - want).max()
            print(f"{form} layers={layers}: max |maps - float64 restatement| = {err:.3e}")
            assert err < 2e-6                                                     # f32 softmax of O(1) scores against float64
            assert (got[~ok] == 0).all()                                          # rows that take no part: exactly 0
            assert np.abs(got.sum(-1) - 1).max() < 1e-5                           # over the context a token's values sum to 1
    finally:
        for layer in pipe.transformer.layers:
            layer.attn2.__dict__.pop("_run_cpu", None)
    assert torch.equal(pipe.tokens2logits(pipe.ids2tokens(ids), context, **kw), plain)


def test_attention_maps_layers_differ_and_arguments_are_checked(pipe, ids):
    context, kw, _, _ = case(pipe, "lens")
    m0, m1, mall = (pipe.attention_maps(ids, context, layers=l, **kw) for l in ([0], [1], None))
    d01, dall = float((m0 - m1).abs().max()), float((mall - m0).abs().max())
    print(f"max |maps(layers=[0]) - maps(layers=[1])| = {d01:.3f}; |maps(all) - maps([0])| = {dall:.3f}")
    assert d01 > 1e-3 and dall > 1e-3
    assert torch.equal(mall, pipe.attention_maps(ids, context, layers=[0, 1], **kw))
    img = torch.rand(B, 3, pipe.image_size, pipe.image_size) * 2 - 1
    _, enc, _ = pipe.to_latent(img)
    assert torch.equal(pipe.attention_maps(img=img, text=context, **kw), pipe.attention_maps(enc.reshape(B, -1), context, **kw))
    prompts = ["a", "b", "c"]
    assert torch.equal(pipe.attention_maps(ids, prompts), pipe.attention_maps(ids, pipe.text_model(prompts)))
    for bad, match in ((dict(layers=[]), "layers"), (dict(layers=[2]), "layers"), (dict(layers=[0, 0]), "layers"), (dict(text=None), "text")):
        with pytest.raises(ValueError, match=match):
            pipe.attention_maps(ids, **{"text": context, **bad})
    with pytest.raises(ValueError, match="exactly one"):
        pipe.attention_maps(text=context)
    with pytest.raises(ValueError, match="exactly one"):
        pipe.attention_maps(ids, context, img=img)


# ------------------------------------------------------------------------------------------------------------------ phrases

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


def _t5(max_length=24):
    return T5TextEmbedder(tokenizer=CharTokenizer(), transformer=tiny_t5(), max_length=max_length)


def test_phrase_rows():
    emb = _t5()
    prompts = ["a red barn here", "barn", "the barn" + "z" * 40]
    calls = []
    tower_forward = emb.transformer.forward
    emb.transformer.forward = lambda *a, **kw: (calls.append(kw["input_ids"].clone()), tower_forward(*a, **kw))[1]
    context, lens, rows = emb.phrase_rows(prompts, ["red barn", "barn", "barn"])
    assert len(calls) == 1                                                                   # ONE tower call
    assert context.shape == (3, 24, 96) and rows.shape == (3, 24) and rows.dtype == torch.bool and lens.dtype == torch.int32
    assert lens.tolist() == [16, 5, 24]
    want = torch.zeros(3, 24, dtype=torch.bool)
    want[0, 2:10], want[1, 0:4], want[2, 4:8] = True, True, True
    assert torch.equal(rows, want)
    assert calls[0][0, :16].tolist() == CharTokenizer.ids_of(prompts[0]) + [1] and calls[0][2, 23] == 1
    # the context of _forward_weighted on the same fragments (the weight syntax only marks them)
    ctx_w, lens_w, _ = emb(["a (red barn:2) here", "(barn:2)", "the (barn:2)" + "z" * 40], weighted=True)
    assert torch.equal(context, ctx_w) and torch.equal(lens, lens_w)
    assert torch.equal(emb.phrase_rows(prompts[:1], "red barn")[2], want[:1])                # one phrase for all
    for prompt, phrase, match in (("a red barn", "cow", "does not occur"), ("barn and barn", "barn", "occurs 2 times"),
                                  ("a red barn", "", "empty"), ("z" * 20 + " barn", "barn", "cut off")):
        with pytest.raises(ValueError, match=match) as e:
            emb.phrase_rows([prompt], [phrase])
        assert repr(prompt) in str(e.value)                                                  # the message names the prompt
    with pytest.raises(ValueError, match="2 phrases"):
        emb.phrase_rows(["a"], ["a", "b"])


def test_the_other_embedders_refuse_phrase_rows():
    with pytest.raises(NotImplementedError, match="phrase"):
        SyntheticTextEmbedder(96).phrase_rows(["a"], ["a"])
    clip = CLIPTextEmbedder(model=StubClipTextTower(), tokenizer=stub_clip_tokenize)
    with pytest.raises(NotImplementedError, match="phrase"):
        clip.phrase_rows(["a"], ["a"])
    with pytest.raises(NotImplementedError, match="phrase"):
        _tiny().phrase_mask(torch.zeros(1, 3, 32, 32), ["a"], "a")


@pytest.fixture(scope="module")
def t5_pipe():
    return _tiny(text_model=T5TextEmbedder(tokenizer=CharTokenizer(), transformer=tiny_t5(), max_length=24))


def test_phrase_mask_is_its_rule_and_edit_keeps_what_is_outside(t5_pipe):
    pipe = t5_pipe
    torch.manual_seed(5)
    img = torch.rand(2, 3, pipe.image_size, pipe.image_size) * 2 - 1
    prompts, phrase = ["a red barn here", "the barn"], ["red barn", "barn"]
    g = pipe.image_size // pipe.patch_size
    context, lens, rows = pipe.text_model.phrase_rows(prompts, phrase)
    maps = pipe.attention_maps(img=img, text=context, context_lens=lens).numpy()
    assert (maps[0, 16:] == 0).all() and (maps[1, 9:] == 0).all()                            # run under the non-pad lengths
    score = (maps * rows.numpy()[:, :, None, None]).sum(1)

    def dilate(m):
        p = np.pad(m, ((0, 0), (1, 1), (1, 1)))
        return np.stack([p[:, 1 + dy:1 + dy + g, 1 + dx:1 + dx + g] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]).any(0)

    for threshold in (0.5, 0.9, 1.0):
        for grow in (0, 1, 2):
            want = score >= np.float32(threshold) * score.max(axis=(1, 2), keepdims=True)
            for _ in range(grow):
                want = dilate(want)
            got = pipe.phrase_mask(img, prompts, phrase, threshold=threshold, grow=grow)
            assert got.dtype == torch.bool and tuple(got.shape) == (2, g, g)
            assert np.array_equal(got.numpy(), want), (threshold, grow)
    one = pipe.phrase_mask(img, prompts, phrase, threshold=1.0)
    assert one.reshape(2, -1).sum(1).tolist() == [1, 1]                                      # the maximum itself
    for bad in (dict(threshold=0), dict(threshold=1.5), dict(grow=-1)):
        with pytest.raises(ValueError):
            pipe.phrase_mask(img, prompts, phrase, **bad)
    # edit under the phrase mask keeps every token outside it
    mask = pipe.phrase_mask(img, prompts, phrase, threshold=0.9)
    assert 0 < int(mask.sum()) < mask.numel()
    _, enc, _ = pipe.to_latent(img)
    _, out_ids = pipe.edit(img, token_mask=mask, text=prompts, timesteps=2, seed=3, return_ids=True)
    keep = ~mask.reshape(2, -1)
    assert torch.equal(out_ids[keep], enc.reshape(2, -1)[keep]) and int((out_ids == pipe.mask_token_id).sum()) == 0
