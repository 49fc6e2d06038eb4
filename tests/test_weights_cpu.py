"""Prompt weights without a GPU: the emphasis parser, the text embedder's weighted mode on a tiny T5 with a
character-level tokenizer, the host checker's messages, the plain-torch branch of ``CrossAttention`` and of a tiny pipeline against
the float64 restatement of tests/weight_ref.py, the duplication property (integer weights = repeated rows), regions with a third
element, ``generate(prompt_weights=True)``, and the proof that the operator data of tests/test_gpu_attention_weights.py bite."""
import numpy as np
import pytest
import torch

import attention_probes as P
import paintmind_amd as pm
import weight_ref as W
from paintmind_amd import ops
from paintmind_amd.generate import Pipeline
from paintmind_amd.modules.attention import CrossAttention
from paintmind_amd.modules.encoder import CLIPTextEmbedder, SyntheticTextEmbedder, T5TextEmbedder
from paintmind_amd.prompt import parse_weighted
from util import load_golden, to_torch_sd

TOL = 1e-3                      # the project's float bar


# ---------------------------------------------------------------------------------------------------------------- the parser

@pytest.mark.parametrize("text,want", [
    ("a red barn", [("a red barn", 1.0)]),
    ("", []),
    ("a (red:1.4) barn, (blurry:0.5)", [("a ", 1.0), ("red", 1.4), (" barn, ", 1.0), ("blurry", 0.5)]),
    ("(a (b:2) c:3)", [("a ", 3.0), ("b", 6.0), (" c", 3.0)]),
    ("((x:2):2) y", [("x", 4.0), (" y", 1.0)]),
    (r"\(x\) 3\:4 (y\::0)", [("(x) 3:4 ", 1.0), ("y:", 0.0)]),
    ("ratio 3:4", [("ratio 3:4", 1.0)]),                       # a colon outside any group is text
    ("(a:1)(b:1)", [("ab", 1.0)]),                             # neighbours of equal weight merge
    ("(a: 2.50 )", [("a", 2.5)]),
    ("back\\slash \\\\", [("back\\slash \\", 1.0)]),
])
def test_parser_cases(text, want):
    assert parse_weighted(text) == want


@pytest.mark.parametrize("text,pos", [
    ("a (red barn", 2), ("a red) barn", 5), ("(red)", 4), ("(red:much)", 5), ("(red:-1)", 5), ("(red:1e3)", 5), ("(red:)", 5),
    ("(a:2", 2), ("(a (b:2)", 0), ("(a:nan)", 3),
])
def test_parser_errors_name_the_position(text, pos):
    with pytest.raises(ValueError, match=f"position {pos}\\b"):
        parse_weighted(text)


# ---------------------------------------------------------------------------------------------------------------- the embedder

class CharTokenizer:
    """one id per character (2 + ord % 100), pad 0, end-of-sequence 1; both call forms the embedder uses"""
    pad_token_id, eos_token_id = 0, 1

    @staticmethod
    def ids_of(s):
        return [2 + ord(c) % 100 for c in s]

    def __call__(self, text, max_length=77, add_special_tokens=True, **kw):
        if isinstance(text, str):
            return {"input_ids": self.ids_of(text) + ([1] if add_special_tokens else [])}
        ids = torch.zeros(len(text), max_length, dtype=torch.long)
        for i, s in enumerate(text):
            row = self.ids_of(s)[:max_length - 1] + [1]
            ids[i, :len(row)] = torch.tensor(row)
        return {"input_ids": ids}


def _t5(d_model=96, max_length=24):
    from transformers import T5Config, T5EncoderModel
    torch.manual_seed(3)
    tower = T5EncoderModel(T5Config(vocab_size=128, d_model=d_model, d_kv=16, d_ff=64, num_layers=1, num_heads=2))
    return T5TextEmbedder(tokenizer=CharTokenizer(), transformer=tower, max_length=max_length)


def test_t5_embedder_weighted_mode():
    emb = _t5()
    prompts = ["a (red:1.4) barn", "(x:0.5)", "z" * 40, "plain"]
    seen = []
    tower_forward = emb.transformer.forward
    emb.transformer.forward = lambda *a, **kw: (seen.append(kw["input_ids"].clone()), tower_forward(*a, **kw))[1]
    context, lens, weights = emb(prompts, weighted=True)
    assert len(seen) == 1                                                                    # ONE tower call
    ids = seen[0]
    assert context.shape == (4, 24, 96) and weights.shape == (4, 24) and weights.dtype == torch.float32
    tok = CharTokenizer.ids_of
    assert ids[0].tolist() == tok("a red barn") + [1] + [0] * 13                              # the syntax is gone, eos closes, pad fills
    assert lens.tolist() == [11, 2, 24, 6]
    assert weights[0].tolist() == pytest.approx([1, 1] + [1.4] * 3 + [1] * 5 + [1] + [1] * 13)   # ... line up with the fragments
    assert ids[1].tolist() == tok("x") + [1] + [0] * 22 and weights[1].tolist() == [0.5] + [1.0] * 23
    assert ids[2].tolist() == tok("z" * 23) + [1]                                              # truncated: the eos stays last
    # a prompt without syntax: the ids, the context and the lens of the unweighted call
    plain_ctx, plain_lens = emb(prompts[3:], return_lens=True)
    assert torch.equal(context[3], plain_ctx[0]) and int(plain_lens[0]) == 6 and bool((weights[3] == 1).all())
    with pytest.raises(ValueError, match="position 0"):
        emb(["(never closed"], weighted=True)


def test_the_other_embedders():
    syn = SyntheticTextEmbedder(96, max_length=8)
    context, lens, weights = syn(["a (b:2)", "c"], weighted=True)
    assert torch.equal(context, syn(["a b", "c"])) and lens.tolist() == [8, 8] and bool((weights == 1).all()) and weights.shape == (2, 8)
    with pytest.raises(ValueError, match="position"):
        syn(["(a"], weighted=True)
    clip = CLIPTextEmbedder.__new__(CLIPTextEmbedder)                                          # (no tower needed to refuse)
    torch.nn.Module.__init__(clip)
    with pytest.raises(NotImplementedError, match="prompt weights"):
        clip.forward(["a"], weighted=True)


# ---------------------------------------------------------------------------------------------------------------- the checker

def test_host_weights_messages():
    B, L, N = 2, 5, 4
    ones = np.ones((B, L), np.float32)
    assert ops.host_weights(None, B, L, N) is None
    cs, ts, w = ops.host_weights(ones.tolist(), B, L, N)
    assert cs.dtype == np.uint8 and (cs == 0).all() and ts.dtype == np.uint32 and (ts == 0xFFFFFFFF).all() and w.dtype == np.float32
    cs, ts, w = ops.host_weights(torch.from_numpy(ones), B, L, N, context_lens=[2, 5])
    assert cs.tolist() == [[0, 0, 255, 255, 255], [0] * 5]
    with pytest.raises(ValueError, match=r"shape \(2, 5\)"):
        ops.host_weights(ones[:, :4], B, L, N)
    for bad in (-1.0, np.nan, np.inf, 2.0 ** -21, 2.0 ** 21):
        x = ones.copy()
        x[1, 3] = bad
        with pytest.raises(ValueError, match=r"image 1: context row 3: weight .* must be 0 or in \[2\^-20, 2\^20\]"):
            ops.host_weights(x, B, L, N)
    x = ones.copy()
    x[0] = 0
    with pytest.raises(ValueError, match="image 0: token 0 allows no context row with a weight above 0"):
        ops.host_weights(x, B, L, N)
    x = ones.copy()
    x[1, :2] = 0
    with pytest.raises(ValueError, match="image 1: token 0 allows no context row"):
        ops.host_weights(x, B, L, N, context_lens=[5, 2])                                   # the live rows lie behind the length
    seg = np.array([[0, 0, 1, 1, 255]] * B)
    tok = np.array([[1, 1, 3, 2]] * B)
    x = ones.copy()
    x[1, 2:4] = 0
    with pytest.raises(ValueError, match="image 1: token 3 allows no context row"):
        ops.host_weights(x, B, L, N, seg, tok)
    with pytest.raises(ValueError, match="exclude each other"):
        ops.host_weights(ones, B, L, N, seg, tok, context_lens=[5, 5])
    with pytest.raises(ValueError, match="come together"):
        ops.host_weights(ones, B, L, N, seg, None)
    x[1, 2] = 2.0 ** 20
    cs, ts, w = ops.host_weights(x, B, L, N, seg, tok)
    assert cs.tolist() == seg.tolist() and w[1, 2] == 2.0 ** 20 and w[1, 3] == 0


# ---------------------------------------------------------------------------------------------------------------- the CPU branch

def _segments(B, N, L, lens):
    ks = np.where(np.arange(L)[None, :] < np.asarray(lens)[:, None], (np.arange(L) // 11 % 3)[None, :], W.PAD).astype(np.uint8)
    qm = (1 | (np.uint32(2) << (np.arange(N, dtype=np.uint32) % 2)[None, :])).repeat(B, 0).astype(np.uint32)      # global + one of two
    return ks, qm


def _weights(B, L, seed=1):
    rng = np.random.default_rng(seed)
    w = rng.choice(np.array([0, 0.125, 1, 8, 1.3, 0.5], np.float32), size=(B, L)).astype(np.float32)
    w[:, :3] = [8, 1, 0.125]
    w[:, 11:13] = [0.5, 8]
    w[:, 22:24] = [1.3, 1]
    return w


@pytest.mark.parametrize("with_segments", [True, False], ids=["segments", "alone"])
def test_cross_attention_cpu_branch_against_the_float64_restatement(with_segments):
    torch.manual_seed(7)
    B, N, L, width = 3, 20, 40, 64
    attn = CrossAttention(width, width, heads=2, dim_head=32).eval()
    g = torch.Generator().manual_seed(5)
    x, ctx = torch.randn(B, N, width, generator=g), 4 * torch.randn(B, L, width, generator=g)
    lens = [40, 33, 25]
    ks, qm = _segments(B, N, L, lens)
    if not with_segments:
        ks, qm = np.where(ks == W.PAD, W.PAD, 0).astype(np.uint8), np.full((B, N), W.ALL, np.uint32)
    w = _weights(B, L)
    want = W.cross_attention(attn, x, ctx, ks, qm, w)
    poisoned = ctx.clone()
    poisoned[torch.from_numpy((ks == W.PAD) | (w == 0))] = float("nan")
    with torch.no_grad():
        if with_segments:
            got = attn.run(x, poisoned, context_segments=ks, token_segments=qm, context_weights=w)
            loose = attn.run(x, torch.nan_to_num(poisoned), context_segments=ks, token_segments=qm)
        else:
            got = attn.run(x, poisoned, context_lens=lens, context_weights=w.tolist())
            loose = attn.run(x, torch.nan_to_num(poisoned), context_lens=lens)
    err, gap = float((got.double().numpy() - want).__abs__().max()), float((loose.double().numpy() - want).__abs__().max())
    print(f"CrossAttention CPU branch, weights {'with segments' if with_segments else 'alone'}: max |torch - float64| = {err:.3e}; "
          f"without the weights {gap:.3e}")
    assert torch.isfinite(got).all() and err < 1e-4 and gap > 100 * TOL


def _tiny():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.eval()


@pytest.fixture(scope="module")
def pipe():
    return _tiny()


def _ref_logits(pipe, tok, context, ks, qm, w):
    """the tiny pipeline's tower in float64 with weight_ref.cross_attention in place of attn2 (everything else plain torch)"""
    tr = pipe.transformer.double()
    try:
        with torch.no_grad():
            h = tr.token_proj(tok.double()) + tr.position_embedding
            c = tr.context_proj(torch.nan_to_num(context).double())
            for layer in tr.layers:
                h = layer.attn1.run(layer.norm1(h), None, residual=h)
                h = h + torch.from_numpy(W.cross_attention(layer.attn2, layer.norm2(h), c, ks, qm, w))
                h = layer.ffnet.run(layer.norm3(h), residual=h)
            return tr.to_logits(tr.norm(h)).float()
    finally:
        pipe.transformer.float()


def test_tokens2logits_cpu_branch_against_the_float64_restatement(pipe):
    B = 3
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, pipe.mask_token_id + 1, (B, pipe.num_tokens), generator=g)
    tok = pipe.ids2tokens(ids)
    context = pipe.text_model(["a", "b", "c"])[:, :40].contiguous()
    lens = [40, 33, 25]
    ks, qm = _segments(B, pipe.num_tokens, 40, lens)
    w = _weights(B, 40)
    context[torch.from_numpy((ks == W.PAD) | (w == 0))] = float("nan")
    want = _ref_logits(pipe, tok, context, ks, qm, w)
    with torch.no_grad():
        got = pipe.tokens2logits(tok, context, context_segments=ks, token_segments=qm, context_weights=w)
        loose = pipe.tokens2logits(tok, torch.nan_to_num(context), context_segments=ks, token_segments=qm)
        ones = pipe.tokens2logits(tok, torch.nan_to_num(context), context_segments=ks, token_segments=qm, context_weights=np.ones_like(w))
    err, gap = float((got - want).abs().max()), float((loose - want).abs().max())
    print(f"tokens2logits CPU branch with weights: max |torch - float64| = {err:.3e}; without the weights {gap:.3e}")
    assert torch.isfinite(got).all() and err < 1e-4 and gap > TOL
    assert float((ones - loose).abs().max()) < 1e-5                                          # weights of 1 change nothing
    # alone and beside lengths: the neutral segments
    ks0 = np.where(ks == W.PAD, W.PAD, 0).astype(np.uint8)
    with torch.no_grad():
        a = pipe.tokens2logits(tok, context, context_lens=lens, context_weights=w)
        b = pipe.tokens2logits(tok, context, context_segments=ks0, token_segments=np.ones((B, pipe.num_tokens), np.uint32), context_weights=w)
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="exclude each other"):
        pipe.tokens2logits(tok, context, context_lens=lens, context_segments=ks, token_segments=qm, context_weights=w)
    with pytest.raises(ValueError, match="text condition"):
        pipe.tokens2logits(tok, None, context_weights=w)


def test_integer_weights_are_repeated_rows():
    """weights 2 and 3 on two rows == the context with those rows repeated, through the existing segmented call"""
    torch.manual_seed(9)
    B, N, L, width = 2, 12, 21, 64
    attn = CrossAttention(width, width, heads=2, dim_head=32).eval()
    g = torch.Generator().manual_seed(6)
    x, ctx = torch.randn(B, N, width, generator=g), 3 * torch.randn(B, L, width, generator=g)
    ks, qm = _segments(B, N, L, [21, 18])
    w = np.ones((B, L), np.float32)
    w[:, 4], w[:, 13] = 2, 3
    dup = torch.cat([ctx, ctx[:, 4:5], ctx[:, 13:14], ctx[:, 13:14]], dim=1)
    ks_dup = np.concatenate([ks, ks[:, 4:5], ks[:, 13:14], ks[:, 13:14]], axis=1)
    with torch.no_grad():
        got = attn.run(x, ctx, context_segments=ks, token_segments=qm, context_weights=w)
        want = attn.run(x, dup, context_segments=ks_dup, token_segments=qm)
        plain = attn.run(x, ctx, context_segments=ks, token_segments=qm)
    assert float((got - want).abs().max()) < 2e-5 and float((plain - want).abs().max()) > 1e-2


# ---------------------------------------------------------------------------------------------------------------- generate

def test_regions_with_a_third_element(pipe):
    g = pipe.image_size // pipe.patch_size
    left = np.zeros((g, g), bool)
    left[:, :g // 2] = True
    texts = ["a", "b"]
    ctx2, ks2, qm2, w2 = pipe._region_context_weighted(texts, [[("d", left)], []], False)
    assert w2 is None                                                                        # two-element items stay as they are
    ctx3, ks3, qm3, w3 = pipe._region_context_weighted(texts, [[("d", left, 0.25)], []], False)
    assert torch.equal(ctx2, ctx3) and np.array_equal(ks2, ks3) and np.array_equal(qm2, qm3)
    assert w3.shape == ks3.shape and (w3[0, :77] == 1).all() and (w3[0, 77:] == 0.25).all() and (w3[1] == 1).all()
    kw = dict(timesteps=3, topk=4, save_interval=1, seed=5, return_ids=True)
    _, ids_w = pipe.generate(texts, regions=[[("d", left, 0.25)], []], **kw)
    opts = pipe._options(4, None, None, None, None, ctx3, 2, None, None, 3)
    _, ids_e = pipe._generate_cpu(ctx3, 2, 3, 1.0, opts, 1, 5, True, ops.host_keys(2, ctx3.shape[1], pipe.num_tokens, None, ks3, qm3, w3))
    assert torch.equal(ids_w, ids_e)
    _, ids_2 = pipe.generate(texts, regions=[[("d", left)], []], **kw)
    _, ids_1 = pipe.generate(texts, regions=[[("d", left, 1.0)], []], **kw)
    assert torch.equal(ids_1, ids_2)                                                         # a weight of 1 is the two-element item
    for bad in ([("d", left, "0.5")], [("d", left, 0.5, 1)], [("d",)], ["d"]):
        with pytest.raises(ValueError, match=r"\(prompt, mask\) pair"):
            pipe.generate(texts, regions=[bad, []], **kw)
    with pytest.raises(ValueError, match=r"weight .* must be 0 or in"):
        pipe.generate(texts, regions=[[("d", left, 2.0 ** 21)], []], **kw)
    with pytest.raises(ValueError, match="no context_weights beside it"):
        pipe.generate(texts, regions=[[("d", left)], []], context_weights=np.ones((2, 154), np.float32), **kw)


def test_prompt_weights_equal_explicit_context_weights(pipe):
    emb = _t5(d_model=96, max_length=24)
    old = pipe.text_model
    pipe.text_model = emb
    try:
        texts = ["a (red:1.4) barn, (blurry:0.5)", "(sky:2) over (sea:0.25)"]
        kw = dict(timesteps=3, topk=4, save_interval=1, seed=5, return_ids=True)
        context, lens, weights = emb(texts, weighted=True)
        assert sorted(set(weights.reshape(-1).tolist())) == pytest.approx([0.25, 0.5, 1.0, 1.4, 2.0])
        for mask_padding in (False, True):
            imgs, ids = pipe.generate(texts, prompt_weights=True, mask_padding=mask_padding, **kw)
            _, want = _explicit(pipe, context, weights, lens if mask_padding else None, kw)
            assert torch.equal(ids, want) and len(imgs) == 3 and torch.isfinite(imgs[-1]).all()
        _, plain = _explicit(pipe, context, None, None, kw)
        assert not torch.equal(plain, want)
        with pytest.raises(ValueError, match="no context_weights beside it"):
            pipe.generate(texts, prompt_weights=True, context_weights=weights, **kw)
        # region prompts are parsed too, and a region's number multiplies its rows' weights
        g = pipe.image_size // pipe.patch_size
        top = np.zeros((g, g), bool)
        top[:g // 2] = True
        _, _, _, w = pipe._region_context_weighted(texts, [[("(x:3) y", top, 0.5)], []], True, True)
        n0 = int(lens[0])
        assert w[0, n0:n0 + 4].tolist() == [1.5, 0.5, 0.5, 0.5] and np.allclose(w[0, :n0], weights[0, :n0].numpy())
        _, ids_r = pipe.generate(texts, prompt_weights=True, mask_padding=True, regions=[[("(x:3) y", top, 0.5)], []], **kw)
        assert ids_r.shape == want.shape
    finally:
        pipe.text_model = old


def _explicit(pipe, context, weights, lens, kw):
    """the CPU loop on an explicit context with explicit weights (what generate builds from the prompts)"""
    B = context.shape[0]
    opts = pipe._options(kw["topk"], None, None, None, None, context, B, None, None, kw["timesteps"])
    seg = None if weights is None else ops.host_keys(B, context.shape[1], pipe.num_tokens, context_lens=lens, context_weights=weights)
    if weights is None and lens is not None:
        opts = opts._replace(lens=list(lens))
    return pipe._generate_cpu(context, B, kw["timesteps"], 1.0, opts, kw["save_interval"], kw["seed"], True, seg)


# ---------------------------------------------------------------------------------------------------------------- the inputs bite

@pytest.mark.parametrize("exp2", [True, False], ids=["exp2", "exp"])
def test_the_operator_data_bite(exp2):
    """the float64 result WITHOUT the weights (same finite inputs, same segments, every weight 1 -- a row of weight 0 attended to)
    misses the weighted bound by more than 100 x in every image at every Nkv > 1, under the bf16 and the f32 bound alike"""
    import region_ref as R
    smallest = {"bf16": np.inf, "f32": np.inf}
    for nkv in W.NKVS:
        d = W.inputs(P.gauss, nkv)
        assert np.isnan(d["k"]).any() or nkv == 1
        unweighted, _, _ = R.attention(d["q"], np.nan_to_num(d["k"]), d["vz"], d["ks"], d["qm"], exp2)
        for kind in smallest:
            ref, Bd, _ = W.bounds(P, d, kind, exp2)
            for b in range(3):
                ratio, _ = P.worst_ratio(unweighted[b], ref[b], Bd[b])
                if nkv == 1:
                    assert ratio <= 1.0                                                    # one key: its weight cancels
                    continue
                assert ratio > 100.0, (kind, nkv, b, ratio)
                smallest[kind] = min(smallest[kind], ratio)
    print(f"exp2={exp2}: smallest (unweighted - weighted) / bound over images and key counts: bf16 {smallest['bf16']:.3g}, f32 {smallest['f32']:.3g}")
