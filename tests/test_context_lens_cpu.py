"""Per-image context lengths without a GPU: the new symbols of the library, the host-side validation of the *_lens entries, the
plain-torch branch of a CPU pipeline (rows at or beyond an image's length never reach a result, NaN included), the embedders'
token counts, ``generate(mask_padding=True)`` and a CPU decode session whose requests bring contexts of different lengths."""
import ctypes as C

import pytest
import torch

import paintmind_amd as pm
from paintmind_amd import _lib, ops
from paintmind_amd.generate import Pipeline
from paintmind_amd.modules.encoder import CLIPTextEmbedder, T5TextEmbedder
from text_stubs import StubClipTextTower, StubTokenizer, stub_clip_tokenize, tiny_t5
from util import load_golden, to_torch_sd

TOL = 1e-3                      # the project's float bar (tests/test_gpu_slots.py)
L, LENS = 77, (1, 33, 64, 77)
NEW = ("pmhip_attention_lens", "pmhip_s2_forward_lens", "pmhip_pipeline_sample_lens", "pmhip_pipeline_generate_lens",
       "pmhip_pipeline_step_slots_lens")


def test_new_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11 == _lib.ABI_VERSION
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None
    header = open(_lib._HERE + "/../include/pmhip.h").read()
    for name in NEW:
        assert f"int {name}(" in header


def test_native_entries_check_host_lengths_before_anything_runs():
    """fake non-null pointers: a call that got past the checks would fault, so every one of these is refused on the host"""
    lib = _lib.load()
    p = C.c_void_p(64)
    arr = lambda *v: (C.c_int * len(v))(*v)
    T1 = ((C.c_float * 1)(1.0), (C.c_int * 1)(1), (C.c_ubyte * 1)(0))
    calls = {
        "s2_forward_lens": lambda lens: lib.pmhip_s2_forward_lens(p, p, p, L, 3, lens, p, None),
        "pipeline_sample_lens": lambda lens: lib.pmhip_pipeline_sample_lens(p, None, p, p, L, 3, lens, 1, 1.0, 1, None, 0, 0, 0, None, None,
                                                                            None, 0, 0.0, None),
        "pipeline_generate_lens": lambda lens: lib.pmhip_pipeline_generate_lens(p, None, p, p, L, 3, lens, 1, *T1, 1, 0, 0, None, 0, None, None,
                                                                                0, None, 0, 0.0),
        "pipeline_step_slots_lens": lambda lens: lib.pmhip_pipeline_step_slots_lens(p, p, p, L, 3, lens, (_lib.Slot * 3)(), None, 0, None, None,
                                                                                    None),
    }
    for who, call in calls.items():
        for lens, image, value in ((arr(5, 0, 7), 1, 0), (arr(5, 6, L + 1), 2, L + 1), (arr(-3, 6, 7), 0, -3)):
            assert call(lens) == _lib.PMHIP_EINVAL, who
            msg = lib.pmhip_last_error().decode()
            assert who in msg and f"image {image}" in msg and str(value) in msg and f"L={L}" in msg, msg
    # lengths without a context
    assert lib.pmhip_s2_forward_lens(p, p, None, 0, 3, arr(1, 1, 1), p, None) == _lib.PMHIP_EINVAL
    assert b"without a context" in lib.pmhip_last_error()
    # the operator entry needs its device lengths
    assert lib.pmhip_attention_lens(0, p, p, p, p, 64, 1, 1, 64, 16, 64, 64, 0, None, None) == _lib.PMHIP_EINVAL
    assert b"kv_lens" in lib.pmhip_last_error()


def test_host_lens_accepts_lists_and_tensors_and_names_the_image():
    assert ops.host_lens(None, 4, L) is None
    assert ops.host_lens([1, 33, 64, 77], 4, L) == [1, 33, 64, 77]
    assert ops.host_lens(torch.tensor([1, 33, 64, 77], dtype=torch.int32), 4, L) == [1, 33, 64, 77]
    for bad, word in (([1, 0, 5, 5], "image 1"), ([1, 2, 3, L + 1], "image 3"), ([1, 2, 3], "3 lengths for a batch of 4"), ([1, 2, 3, 4.5], "image 3")):
        with pytest.raises(ValueError, match=word):
            ops.host_lens(bad, 4, L)


@pytest.fixture(scope="module")
def pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("text_model")]
    return pipe


@pytest.fixture(scope="module")
@torch.no_grad()
def case(pipe):
    """B = 4 contexts of 77 rows with lengths (1, 33, 64, 77), tokens of a half-masked state, and the logits of every image with
    its context CUT to its length, run at the same B (the other rows carry the same cut context: rows never mix)"""
    B, N = len(LENS), pipe.num_tokens
    g = torch.Generator().manual_seed(3)
    ctx = pipe.text_model(["w", "x", "y", "z"]).clone()
    ids = torch.randint(0, pipe.mask_token_id, (B, N), generator=g)
    ids[torch.rand(B, N, generator=g) < 0.5] = pipe.mask_token_id
    tok = pipe.ids2tokens(ids)
    cut = torch.stack([pipe.tokens2logits(tok, ctx[b:b + 1, :n].expand(B, n, -1))[b] for b, n in enumerate(LENS)])

    def padded(fill):
        c = ctx.clone()
        for b, n in enumerate(LENS):
            c[b, n:] = fill(L - n, c.shape[2])
        return c
    return dict(B=B, ctx=ctx, ids=ids, tok=tok, cut=cut, padded=padded, g=g)


def _fills(g):
    return {"zeros": lambda r, d: torch.zeros(r, d), "large": lambda r, d: 50 * torch.randn(r, d, generator=g),
            "nan": lambda r, d: torch.full((r, d), float("nan"))}


@torch.no_grad()
def test_cpu_logits_equal_the_truncated_context_and_ignore_the_padding(pipe, case):
    outs = {name: pipe.tokens2logits(case["tok"], case["padded"](fill), context_lens=list(LENS)) for name, fill in _fills(case["g"]).items()}
    for name, out in outs.items():
        assert torch.isfinite(out).all(), name
        assert torch.equal(out, outs["zeros"]), name                       # NaN-poisoned padding changes nothing
    err = float((outs["nan"] - case["cut"]).abs().max())
    print(f"CPU: max |logits(context, lens) - logits(truncated context)| = {err:.3e}")
    assert err < TOL
    # a tensor of lengths is as good as a list, and the full length IS the call without lengths
    assert torch.equal(pipe.tokens2logits(case["tok"], case["ctx"], context_lens=torch.tensor(LENS)), outs["zeros"])
    assert torch.equal(pipe.tokens2logits(case["tok"], case["ctx"], context_lens=[L] * 4), pipe.tokens2logits(case["tok"], case["ctx"]))
    # the counter-check: without lengths the padding IS text, and large padding moves the logits far beyond the bar
    loud = pipe.tokens2logits(case["tok"], case["padded"](_fills(case["g"])["large"]))
    gap = float((loud[:3] - case["cut"][:3]).abs().max())
    print(f"CPU: the same padding without lengths moves the logits by {gap:.3e}")
    assert gap > 100 * TOL
    assert float((loud[3] - case["cut"][3]).abs().max()) < TOL            # the image that fills its context has no padding


def test_cpu_sample_and_generate_ids_equal_the_truncated_context(pipe, case):
    B = case["B"]
    nan_ctx = case["padded"](_fills(case["g"])["nan"])
    noise = torch.rand(B, pipe.num_tokens, pipe.mask_token_id, generator=case["g"])
    got, img = pipe.sample(case["ids"], 0.5, text=nan_ctx, topk=3, temperature=0.8, noise=noise, context_lens=list(LENS))
    assert torch.isfinite(img).all()
    for b, n in enumerate(LENS):
        want, _ = pipe.sample(case["ids"], 0.5, text=case["ctx"][b:b + 1, :n].expand(B, n, -1), topk=3, temperature=0.8, noise=noise)
        assert torch.equal(got[b], want[b]), b
    # the guided step: only the conditional forward sees lengths
    g1, _ = pipe.sample(case["ids"], 0.5, text=nan_ctx, topk=3, temperature=0.8, noise=noise, context_lens=list(LENS), guidance_scale=2.0)
    for b, n in enumerate(LENS):
        want, _ = pipe.sample(case["ids"], 0.5, text=case["ctx"][b:b + 1, :n].expand(B, n, -1), topk=3, temperature=0.8, noise=noise,
                              guidance_scale=2.0)
        assert torch.equal(g1[b], want[b]), b


@torch.no_grad()
def test_cpu_length_validation(pipe, case):
    tok, ctx = case["tok"], case["ctx"]
    for bad in ([0, 5, 5, 5], [5, 5, 5, L + 1], [5, 5, 5], torch.tensor([5, 5, 5, 5, 5])):
        with pytest.raises(ValueError, match="context_lens"):
            pipe.tokens2logits(tok, ctx, context_lens=bad)
        with pytest.raises(ValueError, match="context_lens"):
            pipe.sample(case["ids"], 0.5, text=ctx, context_lens=bad)
    with pytest.raises(ValueError, match="needs a text condition"):
        pipe.tokens2logits(tok, None, context_lens=[1, 1, 1, 1])


TEXTS = ["a", "a cat", "", "x" * 200, "a photo of a dog on a skateboard"]


def test_embedders_return_the_non_pad_token_counts():
    t5 = T5TextEmbedder(tokenizer=StubTokenizer(), transformer=tiny_t5(96))
    ctx, lens = t5(TEXTS, return_lens=True)
    want = (StubTokenizer()(TEXTS, max_length=77)["input_ids"] != 0).sum(-1)
    assert lens.dtype == torch.int32 and lens.device.type == "cpu" and lens.tolist() == want.tolist() == [2, 6, 1, 77, 33]
    assert torch.equal(ctx, t5(TEXTS)) and ctx.shape == (5, 77, 96)
    clip = CLIPTextEmbedder(model=StubClipTextTower(width=96), tokenizer=stub_clip_tokenize)
    ctx, lens = clip(TEXTS, return_lens=True)
    assert lens.tolist() == (stub_clip_tokenize(TEXTS) != 0).sum(-1).tolist() == [2, 6, 1, 77, 33]
    assert torch.equal(ctx, clip(TEXTS))


def test_generate_mask_padding_uses_the_embedders_lengths():
    emb = T5TextEmbedder(tokenizer=StubTokenizer(), transformer=tiny_t5(96))
    torch.manual_seed(4)
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False, text_model=emb).eval()
    texts = TEXTS[:2] + TEXTS[4:]
    ctx, lens = emb(texts, return_lens=True)
    kw = dict(timesteps=3, topk=3, save_interval=1, seed=5, return_ids=True)
    imgs_m, ids_m = pipe.generate(texts, mask_padding=True, **kw)
    imgs_l, ids_l = pipe.generate(texts, context_lens=lens, **kw)
    assert torch.equal(ids_m, ids_l) and all(torch.equal(a, b) for a, b in zip(imgs_m, imgs_l))
    # the default is the reference's behaviour: every row of the padded context is attended to
    imgs_d, ids_d = pipe.generate(texts, **kw)
    imgs_f, ids_f = pipe.generate(texts, context_lens=[77] * 3, **kw)
    assert torch.equal(ids_d, ids_f) and all(torch.equal(a, b) for a, b in zip(imgs_d, imgs_f))
    assert not all(torch.equal(a, b) for a, b in zip(imgs_d, imgs_m))     # the padding of a T5 context is not nothing
    # one step of the masked loop is the step on the truncated contexts
    ids0 = torch.full((3, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long)
    noise = torch.rand(3, pipe.num_tokens, pipe.mask_token_id, generator=torch.Generator().manual_seed(1))
    got, _ = pipe.sample(ids0, 0.5, text=ctx, topk=3, noise=noise, context_lens=lens)
    for b, n in enumerate(lens.tolist()):
        want, _ = pipe.sample(ids0, 0.5, text=ctx[b:b + 1, :n].expand(3, n, -1), topk=3, noise=noise)
        assert torch.equal(got[b], want[b]), b


# (prompt, context rows, T, temperature, topk, seed, guidance scale)
REQUESTS = [("a", 1, 3, 1.0, 5, 11, None), ("b", 33, 5, 0.7, 3, 22, 2.0), ("c", 64, 4, 1.3, 1, 33, None), ("d", 77, 3, 0.9, 8, 44, 1.5),
            ("e", 40, 4, 0.5, 2, 55, None)]


def test_cpu_session_with_mixed_context_lengths_equals_generate_alone(pipe):
    s = pipe.decode_session(slots=2, conditional=True, max_context_len=77)
    full = {tx: pipe.text_model([tx])[0] for tx, *_ in REQUESTS}
    for tx, n, T, temp, k, seed, scale in REQUESTS:
        s.submit(context=full[tx][:n], timesteps=T, temperature=temp, topk=k, seed=seed, guidance_scale=scale)
    with pytest.raises(ValueError, match="max_context_len"):
        s.submit(context=torch.zeros(78, 96))
    done = s.drain()
    assert sorted(f.handle.number for f in done) == [0, 1, 2, 3, 4]
    for f in done:
        tx, n, T, temp, k, seed, scale = REQUESTS[f.handle.number]
        imgs, ids = pipe.generate([tx], timesteps=T, temperature=temp, topk=k, save_interval=1, seed=seed, return_ids=True,
                                  guidance_scale=scale, context_lens=[n])
        assert torch.equal(f.ids, ids[0]), f.handle
        assert torch.equal(f.image, imgs[-1][0]), f.handle
