"""Regional prompts without a GPU: the new symbols of the library and the host-side validation of the
*_segments entries, the plain-torch branch of ``CrossAttention`` against the float64 restatement of tests/region_ref.py, the
Pipeline surface on a CPU pipeline (``tokens2logits`` / ``sample`` / ``generate(regions=)``), every ValueError, and the
pixel-to-token rule."""
import ctypes as C

import numpy as np
import pytest
import torch

import paintmind_amd as pm
import region_ref as R
from paintmind_amd import _lib, ops
from paintmind_amd.generate import MAX_REGIONS, Pipeline, region_layout, region_token_mask
from util import load_golden, to_torch_sd

TOL = 1e-3                      # the project's float bar (tests/test_context_lens_cpu.py)
NEW = ("pmhip_attention_segments", "pmhip_s2_forward_segments", "pmhip_pipeline_sample_segments", "pmhip_pipeline_generate_segments")
B = 3


def test_new_symbols_are_exported_and_the_abi_version_stays():
    lib = _lib.load()
    assert lib.pmhip_abi_version() == 11 == _lib.ABI_VERSION
    header = open(_lib._HERE + "/../include/pmhip.h").read()
    for name in NEW:
        assert name in _lib.PROTOTYPES and getattr(lib, name) is not None
        assert f"int {name}(" in header


def test_native_entries_check_host_segments_before_anything_runs():
    """A handle made on the host (creating one launches nothing and touches no device) and fake non-null pointers everywhere else: a
    call that got past the checks would fault, so every one of these is refused before anything runs."""
    lib = _lib.load()
    p = C.c_void_p(64)
    L, N = 5, 16
    cfg = _lib.S2Cfg(N, 32, 64, 128, 128, _lib.TowerCfg(128, 0, 2, 256, 64))
    handle = C.c_void_p()
    assert lib.pmhip_s2_create(C.byref(handle), 0, _lib.F32, C.byref(cfg), C.byref(_lib.S2Weights())) == _lib.PMHIP_OK
    T1 = ((C.c_float * 1)(1.0), (C.c_int * 1)(1), (C.c_ubyte * 1)(0))
    seg = lambda rows: (C.c_ubyte * (B * L))(*[v for r in rows for v in r])
    tok = lambda rows: (C.c_uint32 * (B * N))(*[v for r in rows for v in r])
    good_seg, good_tok = [[0, 1, 1, 255, 255]] * B, [[1] * N] * B
    calls = {
        "s2_forward_segments": lambda s, t, ctx=p, L=L, lens=None: lib.pmhip_s2_forward_segments(handle, p, ctx, L, B, s, t, p, None),
        "pipeline_sample_segments": lambda s, t, ctx=p, L=L, lens=None: lib.pmhip_pipeline_sample_segments(
            handle, None, p, ctx, L, B, lens, 1, 1.0, 1, None, 0, 0, 0, None, None, None, 0, 0.0, 0.0, None, 1.0, None, 0, None, s, t, None),
        "pipeline_generate_segments": lambda s, t, ctx=p, L=L, lens=None: lib.pmhip_pipeline_generate_segments(
            handle, None, p, ctx, L, B, lens, 1, *T1, 1, 0, 0, None, 0, None, None, 0, None, 0, 0.0, None, 1.0, None, 0, None, None, s, t),
    }
    bad_id = [r[:] for r in good_seg]
    bad_id[1][2] = 32
    no_key = [r[:] for r in good_tok]
    no_key[2][9] = 0b100                                                 # segment 2: no row of the image has it
    only_pad = [[255] * L] + good_seg[1:]
    try:
        for who, call in calls.items():
            for s, t_, words in ((seg(good_seg), None, ("come together",)), (None, tok(good_tok), ("come together",)),
                                 (seg(bad_id), tok(good_tok), ("image 1", "context row 2", "segment 32")),
                                 (seg(good_seg), tok(no_key), ("image 2", "token 9", "allows no segment")),
                                 (seg(only_pad), tok(good_tok), ("image 0", "token 0", "allows no segment"))):
                assert call(s, t_) == _lib.PMHIP_EINVAL, (who, words)
                msg = lib.pmhip_last_error().decode()
                assert who in msg and all(w in msg for w in words), msg
            assert call(seg(good_seg), tok(good_tok), ctx=None, L=0) == _lib.PMHIP_EINVAL, who        # segments without a context
            assert b"without a context" in lib.pmhip_last_error()
        for who in ("pipeline_sample_segments", "pipeline_generate_segments"):      # segments beside lengths
            assert calls[who](seg(good_seg), tok(good_tok), lens=(C.c_int * B)(5, 5, 5)) == _lib.PMHIP_EINVAL
            assert b"exclude" in lib.pmhip_last_error()
    finally:
        lib.pmhip_s2_destroy(handle)
    # the operator entry needs its device arrays
    assert lib.pmhip_attention_segments(0, p, p, p, p, 64, 1, 1, 64, 16, 64, 64, 0, None, p, None) == _lib.PMHIP_EINVAL
    assert b"key_seg" in lib.pmhip_last_error()
    assert lib.pmhip_attention_segments(0, p, p, p, p, 64, 1, 1, 64, 16, 64, 64, 0, p, None, None) == _lib.PMHIP_EINVAL


def test_host_segments_names_the_image_and_the_token():
    assert ops.host_segments(None, None, 2, 4, 3) is None
    cs, ts = ops.host_segments([[0, 1, -1, 255], [0, 0, 31, 255]], torch.tensor([[1, 3, 2], [1, 1 << 31, 1]]), 2, 4, 3)
    assert cs.dtype == np.uint8 and cs.tolist() == [[0, 1, 255, 255], [0, 0, 31, 255]]
    assert ts.dtype == np.uint32 and ts.tolist() == [[1, 3, 2], [1, 1 << 31, 1]]
    ok = ops.segments_allowed(cs, ts)
    assert np.array_equal(ok, R.allowed(cs, ts))
    good_c, good_t = [[0, 1, 255, 255], [0, 0, 31, 255]], [[1, 3, 2], [1, 1, 1]]
    for c, t_, word in ((good_c, None, "come together"), (None, good_t, "come together"),
                        ([[0, 1, 32, 255], [0, 0, 0, 0]], good_t, "image 0: context row 2: segment 32"),
                        ([[0, 1, 1, 1], [0, -2, 0, 0]], good_t, "image 1: context row 1: segment -2"),
                        (good_c, [[1, 3, 2], [1, 2, 1]], "image 1: token 1 allows no segment"),
                        (good_c, [[1, 3, 0], [1, 1, 1]], "image 0: token 2 allows no segment"),
                        (good_c, [[1, 3, 2]], "token_segments must be"), ([[0, 1, 2]], good_t, "context_segments must be"),
                        (good_c, [[1.0, 3, 2], [1, 1, 1]], "token_segments must be"), (good_c, [[1, -3, 2], [1, 1, 1]], "32-bit mask")):
        with pytest.raises(ValueError, match=word):
            ops.host_segments(c, t_, 2, 4, 3)


@pytest.fixture(scope="module")
def pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False).eval()
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not [k for k in missing.missing_keys if not k.startswith("text_model")]
    return pipe


def _masks(pipe):
    """left half (a pixel mask), bottom-right quadrant plus one stray pixel (a pixel mask that only the any-pixel rule turns into
    that token), and a token mask overlapping both"""
    S, g = pipe.image_size, pipe.image_size // pipe.patch_size
    left = torch.zeros(S, S, dtype=torch.uint8)
    left[:, :S // 2] = 1
    corner = torch.zeros(S, S)
    corner[S // 2:, S // 2:] = 0.5
    corner[3, S - 2] = 1.0                                   # one pixel of the top-right token
    tm = torch.zeros(g, g, dtype=torch.bool)
    tm[1:3, 1:3] = True
    return left, corner, tm


@pytest.fixture(scope="module")
@torch.no_grad()
def case(pipe):
    """B = 3: image 0 with two regions, image 1 with one, image 2 with none -- their totals differ, so images 1 and 2 carry padding"""
    left, corner, tm = _masks(pipe)
    g = torch.Generator().manual_seed(3)
    N = pipe.num_tokens
    glob = pipe.text_model(["g0", "g1", "g2"]).clone()                             # [3, 77, 96]
    extra = pipe.text_model(["r", "s", "t", "u", "v", "w"]).clone()[3:]            # other rows than the global prompts'
    regions = [[(extra[0, :40], left), (extra[1, :9], corner)], [(extra[2, :25], tm)], []]
    context, ks, qm = R.layout([glob[b] for b in range(B)], regions, pipe.image_size, pipe.patch_size)
    ids = torch.randint(0, pipe.mask_token_id, (B, N), generator=g)
    ids[torch.rand(B, N, generator=g) < 0.5] = pipe.mask_token_id
    return dict(context=context, ks=ks, qm=qm, ids=ids, tok=pipe.ids2tokens(ids), glob=glob, regions=regions, g=g)


def test_the_layout_of_the_package_is_the_restatements(pipe, case):
    contexts = [[case["glob"][b]] + [rows for rows, _ in case["regions"][b]] for b in range(B)]
    context, ks, qm = region_layout(contexts, [[m for _, m in case["regions"][b]] for b in range(B)], pipe.image_size, pipe.patch_size)
    assert torch.equal(context, case["context"]) and np.array_equal(ks, case["ks"]) and np.array_equal(qm, case["qm"])
    assert context.shape[1] == 77 + 40 + 9 and (ks[2, 77:] == 255).all() and (ks[1, 77 + 25:] == 255).all()
    assert qm[2].tolist() == [1] * pipe.num_tokens                                  # no region: the global prompt only
    assert qm[0].tolist() == [3, 3, 1, 5, 3, 3, 1, 1, 3, 3, 5, 5, 3, 3, 5, 5]       # the stray pixel makes token 3 part of region 2


def test_pixel_to_token_rule_agrees_with_edit(pipe):
    S, p = pipe.image_size, pipe.patch_size
    g = torch.Generator().manual_seed(9)
    for density in (0.002, 0.02, 0.5):
        pmask = (torch.rand(S, S, generator=g) < density).to(torch.uint8)
        want = pmask.reshape(1, S // p, p, S // p, p).amax(dim=(2, 4)).reshape(-1) != 0          # the expression of Pipeline.edit
        _, pm_ = pipe._edit_masks(torch.zeros(1, 3, S, S), pmask, None)
        assert torch.equal(pm_[0], pmask)
        got = region_token_mask(pmask, S, p)
        assert torch.equal(got, want) and np.array_equal(got.numpy(), R.token_mask_of(pmask.numpy(), S, p))
    tm = torch.rand(S // p, S // p, generator=g) < 0.5
    assert torch.equal(region_token_mask(tm, S, p), tm.reshape(-1))
    with pytest.raises(ValueError, match="a mask must be"):
        region_token_mask(torch.zeros(S, S + 1), S, p)


@torch.no_grad()
def test_run_cpu_against_the_float64_restatement(pipe, case):
    attn = pipe.transformer.layers[0].attn2
    g = case["g"]
    x = torch.randn(B, pipe.num_tokens, attn.query_dim, generator=g)
    ctx = torch.randn(B, case["ks"].shape[1], attn.context_dim, generator=g)
    want = R.cross_attention(attn, x, ctx, case["ks"], case["qm"])
    got = attn.run(x, ctx, context_segments=case["ks"], token_segments=case["qm"])
    err = float((got.double() - want).abs().max())
    gap = float((attn.run(x, ctx).double() - want).abs().max())
    print(f"CPU CrossAttention: max |masked - float64| = {err:.3e}; without the masks {gap:.3e}")
    assert err < TOL and gap > 100 * TOL
    # NaN in the padding rows changes nothing, bit for bit; lists and tensors are as good as arrays
    poisoned = ctx.clone()
    poisoned[torch.from_numpy(case["ks"] == 255)] = float("nan")
    assert torch.equal(attn.run(x, poisoned, context_segments=case["ks"].tolist(), token_segments=torch.from_numpy(case["qm"].astype(np.int64))), got)
    with pytest.raises(ValueError, match="need a context"):
        attn.run(x, None, context_segments=case["ks"], token_segments=case["qm"])
    with pytest.raises(ValueError, match="exclude"):
        attn.run(x, ctx, context_lens=[5, 5, 5], context_segments=case["ks"], token_segments=case["qm"])


@torch.no_grad()
def test_every_token_allowing_every_segment_is_the_call_without_segments(pipe, case):
    ctx = case["context"][:, :117]                                                  # rows every image has text in ...
    ks = np.minimum(case["ks"][:, :117], 31)                                        # ... (image 2's padding taken as text: zeros)
    every = np.full((B, pipe.num_tokens), 0xFFFFFFFF, np.uint32)
    assert torch.equal(pipe.tokens2logits(case["tok"], ctx, context_segments=ks, token_segments=every), pipe.tokens2logits(case["tok"], ctx))
    noise = torch.rand(B, pipe.num_tokens, pipe.mask_token_id, generator=case["g"])
    a = pipe.sample(case["ids"], 0.5, text=ctx, topk=3, noise=noise, context_segments=ks, token_segments=every, guidance_scale=2.0)
    b = pipe.sample(case["ids"], 0.5, text=ctx, topk=3, noise=noise, guidance_scale=2.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@torch.no_grad()
def test_padding_rows_never_reach_the_logits_and_a_token_sees_its_regions_only(pipe, case):
    outs = {}
    for name, fill in (("zeros", 0.0), ("large", 1e30), ("nan", float("nan"))):
        ctx = case["context"].clone()
        ctx[torch.from_numpy(case["ks"] == 255)] = fill
        outs[name] = pipe.tokens2logits(case["tok"], ctx, context_segments=case["ks"], token_segments=case["qm"])
        assert torch.isfinite(outs[name]).all(), name
        assert torch.equal(outs[name], outs["zeros"]), name
    # image 2 has no region: its logits are those of its global prompt alone; images 0 and 1 move when their regions' text does
    alone = pipe.tokens2logits(case["tok"], case["glob"])
    assert float((outs["zeros"][2] - alone[2]).abs().max()) < TOL
    other = case["context"].clone()
    other[:, 77:] = torch.randn(other[:, 77:].shape, generator=case["g"])
    moved = pipe.tokens2logits(case["tok"], other, context_segments=case["ks"], token_segments=case["qm"])
    assert float((moved[2] - outs["zeros"][2]).abs().max()) < TOL
    assert float((moved[0] - outs["zeros"][0]).abs().max()) > 100 * TOL and float((moved[1] - outs["zeros"][1]).abs().max()) > 100 * TOL
    # the counter-check: without the arrays the same context gives other logits, far beyond the bar
    assert float((pipe.tokens2logits(case["tok"], case["context"]) - outs["zeros"]).abs().max()) > 100 * TOL


class _Rows(torch.nn.Module):
    """a text model whose prompts name their rows: "name:count" -> the first `count` of 77 rows of N(0, 1) keyed by the name"""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def rows(self, prompt):
        name, count = prompt.split(":")
        g = torch.Generator().manual_seed(sum(ord(c) * 131 ** i for i, c in enumerate(name)))
        full = torch.randn(77, self.dim, generator=g)
        full[int(count):] = 7.0                                                     # "padding": loud, so that masking it matters
        return full, int(count)

    def forward(self, text, return_lens=False):
        got = [self.rows(p) for p in text]
        ctx = torch.stack([r for r, _ in got])
        return (ctx, torch.tensor([c for _, c in got], dtype=torch.int32)) if return_lens else ctx


@pytest.fixture(scope="module")
def rows_pipe(pipe):
    torch.manual_seed(4)
    rp = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False, text_model=_Rows(96)).eval()
    rp.load_state_dict({k: v for k, v in pipe.state_dict().items() if not k.startswith("text_model")}, strict=False)
    return rp


def test_one_region_covering_the_grid_is_the_concatenated_context(rows_pipe):
    """generate(text, regions=[one region over every token]) == the loop on [global | region] without masks: exact ids and images.
    With mask_padding every prompt contributes its non-pad rows only."""
    pipe = rows_pipe
    S = pipe.image_size
    texts, reg = ["a:77", "b:77"], ["c:77", "d:77"]
    kw = dict(timesteps=3, topk=3, save_interval=1, seed=5, return_ids=True)
    imgs, ids = pipe.generate(texts, regions=[[(r, torch.ones(S, S))] for r in reg], **kw)
    cat = torch.cat([pipe.text_model(texts), pipe.text_model(reg)], dim=1)
    opts = pipe._options(3, None, None, None, None, cat, 2, timesteps=3)
    imgs_c, ids_c = pipe._generate_cpu(cat, 2, 3, 1.0, opts, 1, 5, True)
    assert torch.equal(ids, ids_c) and all(torch.equal(a, b) for a, b in zip(imgs, imgs_c))
    # mask_padding: prompts of 20 / 30 and 5 / 77 non-pad rows -> totals 25 and 107, image 0 padded (zero-filled) to 107
    texts, reg = ["a:20", "b:30"], ["c:5", "d:77"]
    imgs, ids = pipe.generate(texts, regions=[[(r, torch.ones(S, S))] for r in reg], mask_padding=True, **kw)
    per_image = []
    for b in range(2):
        cat = torch.cat([pipe.text_model([texts[b]])[0, :int(texts[b].split(":")[1])], pipe.text_model([reg[b]])[0, :int(reg[b].split(":")[1])]])[None]
        opts = pipe._options(3, None, None, None, None, cat.expand(2, -1, -1), 2, timesteps=3)
        per_image.append(pipe._generate_cpu(cat.expand(2, -1, -1), 2, 3, 1.0, opts, 1, 5, True)[1][b])
    assert torch.equal(ids, torch.stack(per_image))
    # and without mask_padding the loud padding rows are text: another result
    assert not torch.equal(pipe.generate(texts, regions=[[(r, torch.ones(S, S))] for r in reg], **kw)[1], ids)


def test_generate_with_regions_composes_with_guidance_and_a_negative_prompt(rows_pipe):
    """the loop with regions is the per-step ``sample`` composition with the same arrays; guidance and a negative prompt act in passes
    that carry no segments"""
    pipe = rows_pipe
    S, g = pipe.image_size, pipe.image_size // pipe.patch_size
    left = torch.zeros(S, S)
    left[:, :S // 2] = 1
    tm = torch.zeros(g, g, dtype=torch.bool)
    tm[2:] = True
    texts = ["a:77", "b:40", "c:10"]
    regions = [[("d:30", left), ("e:12", tm)], [("f:77", tm)], []]
    context, ks, qm = pipe._region_context(texts, regions, True)
    assert context.shape == (3, 77 + 30 + 12, 96) and (ks[2, 10:] == 255).all() and (context[2, 10:] == 0).all()
    for kw in (dict(), dict(guidance_scale=3.0), dict(guidance_scale=3.0, negative_text="n:33")):
        imgs, ids = pipe.generate(texts, timesteps=3, topk=3, save_interval=1, seed=5, return_ids=True, regions=regions, mask_padding=True, **kw)
        temps, nmask = pipe._schedule(3, 1.0)
        step_ids = torch.full((3, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long)
        skw = dict(kw)
        if "negative_text" in skw:
            neg, lens = pipe.text_model(["n:33"] * 3, return_lens=True)
            skw.update(negative_text=neg, negative_context_lens=lens)
        for step in range(3):
            opts = pipe._options(3, None, skw.get("guidance_scale"), None, None, context, 3, skw.get("negative_text"), skw.get("negative_context_lens"))
            step_ids, img = pipe._step(step_ids, nmask[step], context, opts, temps[step], 0.0, seed=5 + step,
                                       keys=ops.host_keys(3, context.shape[1], pipe.num_tokens, None, ks, qm))
            assert torch.equal(img, imgs[step]), (kw, step)
        assert torch.equal(step_ids, ids), kw
    plain = pipe.generate(texts, timesteps=3, topk=3, save_interval=1, seed=5, return_ids=True)[1]
    assert not torch.equal(plain, ids)


def test_every_value_error(pipe, case, rows_pipe):
    tok, ctx, ks, qm = case["tok"], case["context"], case["ks"], case["qm"]
    S = pipe.image_size
    one = torch.ones(S, S)
    with pytest.raises(ValueError, match="needs? a text condition"):
        pipe.tokens2logits(tok, None, context_segments=ks, token_segments=qm)
    with pytest.raises(ValueError, match="exclude"):
        pipe.tokens2logits(tok, ctx, context_lens=[5, 5, 5], context_segments=ks, token_segments=qm)
    with pytest.raises(ValueError, match="come together"):
        pipe.tokens2logits(tok, ctx, context_segments=ks)
    bad = ks.copy().astype(np.int64)
    bad[1, 4] = 40
    with pytest.raises(ValueError, match="image 1: context row 4: segment 40"):
        pipe.tokens2logits(tok, ctx, context_segments=bad, token_segments=qm)
    none = qm.copy()
    none[0, 7] = 1 << 9                                               # a segment no row of image 0 has
    with pytest.raises(ValueError, match="image 0: token 7 allows no segment"):
        pipe.sample(case["ids"], 0.5, text=ctx, context_segments=ks, token_segments=none)
    with pytest.raises(ValueError, match="context_segments must be"):
        pipe.sample(case["ids"], 0.5, text=ctx, context_segments=ks[:, :5], token_segments=qm)
    rp = rows_pipe
    with pytest.raises(ValueError, match=f"at most {MAX_REGIONS} per image"):
        rp.generate(["a:5"], regions=[[("b:5", one)] * (MAX_REGIONS + 1)], timesteps=2)
    with pytest.raises(ValueError, match="2 lists for a batch of 1"):
        rp.generate(["a:5"], regions=[[], []], timesteps=2)
    with pytest.raises(ValueError, match=r"\(prompt, mask\) pair"):
        rp.generate(["a:5"], regions=[["b:5"]], timesteps=2)
    with pytest.raises(ValueError, match="a mask must be"):
        rp.generate(["a:5"], regions=[[("b:5", torch.ones(3, 3))]], timesteps=2)
    with pytest.raises(ValueError, match="regions builds"):
        rp.generate(["a:5"], regions=[[("b:5", one)]], context_lens=[5], timesteps=2)
    with pytest.raises(TypeError, match="regions"):                   # edit keeps its signature: the keyword does not exist there
        rp.edit(torch.zeros(1, 3, S, S), mask=one, text=["a:5"], regions=[[("b:5", one)]])
    session = rp.decode_session(slots=2, conditional=True)
    with pytest.raises(ValueError, match="regional prompts"):
        session.submit(text="a:5", regions=[("b:5", one)])
    assert rp.generate(["a:5"], regions=[[("b:5", one)] * MAX_REGIONS], timesteps=1, save_interval=1)[0].shape[0] == 1
