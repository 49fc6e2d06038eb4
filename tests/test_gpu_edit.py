"""The region-preserving edit on the MI355X: the re-masking kernels with a count per image against the pinned
single-row calls, the two pixel-side operators against numpy, the native edit loop (eager, captured, replayed with other masks)
against the composition of pinned operators, its tie to the pinned decode loop, and the invariants at full size.  Every comparison
is exact."""
import numpy as np
import pytest
import torch

import paintmind_amd as pm
from edit_ref import (MASK_ID, composed_edit, composite_np, mask_tokens_np, remask_counts_np, scores_with_ties)
from gpu_common import dev, n, scaled_chain_pipeline, t
from negative_ref import PromptRows
from paintmind_amd import ops
from paintmind_amd.generate import Pipeline, edit_schedule, loop_schedule
from util import load_golden, to_torch_sd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tiny():
    p, _ = load_golden("tiny_pipeline.npz")
    cfg = pm.Config(pm.ver2cfg["tiny-pipeline"])
    pipe = Pipeline(cfg, stage1_pretrained=False, text_model=PromptRows(cfg.context_dim, 7, 3))
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.to(dev()).eval()


# ---------------------------------------------------------------------------------------------------------------------------------
# the operator: a count per image
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [16, 1000, 1024])
def test_remask_counts_equals_the_single_row_calls(N):
    B = 5
    counts = [0, 1, N // 3, N - 1, N]
    ids_np, scores_np = scores_with_ties(B, N, seed=N)
    ids, scores = t(ids_np), t(scores_np)
    cd = torch.tensor(counts, dtype=torch.int32, device=dev())
    got = ops.remask_counts(ids.clone(), scores, cd, MASK_ID)
    for b, c in enumerate(counts):
        want = ids[b:b + 1].clone() if c == 0 else ops.remask(ids[b:b + 1].clone(), scores[b:b + 1].clone(), c, MASK_ID)
        assert torch.equal(got[b:b + 1], want), (N, b, c)
    assert torch.equal(got[0], ids[0])                                             # count 0: the row as it was
    assert np.array_equal(n(got), remask_counts_np(ids_np, scores_np, counts, MASK_ID))
    assert int((got[4] == MASK_ID).sum()) == N and int((got[1] == MASK_ID).sum()) == 1
    # the choice form: given noise, then Philox, the noise of image b at row_base + b * N
    u = torch.rand(B, N, generator=torch.Generator().manual_seed(N)).to(dev())
    base = 3 * N
    for noise in (u, None):
        got = ops.remask_counts(ids.clone(), scores, cd, MASK_ID, choice_temperature=4.5, noise=noise, seed=11, step=2, row_base=base)
        for b, c in enumerate(counts):
            want = ids[b:b + 1].clone()
            if c:
                ops.remask(want, scores[b:b + 1].clone(), c, MASK_ID, choice_temperature=4.5, noise=None if noise is None else u[b:b + 1].clone(),
                           seed=11, step=2, row_base=base + b * N)
            assert torch.equal(got[b:b + 1], want), (N, b, c, noise is None)
    # choice temperature 0 without noise IS the plain form
    assert torch.equal(ops.remask_counts(ids.clone(), scores, cd, MASK_ID, choice_temperature=0.0),
                       ops.remask_counts(ids.clone(), scores, cd, MASK_ID))


@pytest.mark.parametrize("N", [16, 300])
def test_remask_counts_above_n_is_the_row_and_a_negative_count_leaves_it(N):
    """the two ends of the count rule the case above does not reach, in the two smallest classes (one and two elements per thread):
    a count above N is pmhip_remask(_choice) on that row alone with that count -- the whole row -- and a negative one leaves the row
    as a 0 does"""
    counts = [N + 5, -3, N + 1]
    ids_np, scores_np = scores_with_ties(3, N, seed=N + 1)
    ids, scores = t(ids_np), t(scores_np)
    cd = torch.tensor(counts, dtype=torch.int32, device=dev())
    base = 3 * N
    for kw in ({}, dict(choice_temperature=4.5, seed=11, step=2)):
        got = ops.remask_counts(ids.clone(), scores, cd, MASK_ID, row_base=base, **kw)
        for b, c in enumerate(counts):
            want = ids[b:b + 1].clone()
            if c > 0:
                ops.remask(want, scores[b:b + 1].clone(), c, MASK_ID, row_base=base + b * N, **kw)
                assert int((want == MASK_ID).sum()) == N, (N, b, c)
            assert torch.equal(got[b:b + 1], want), (N, b, c, kw)
        assert torch.equal(got[1], ids[1])                                         # a negative count: the row as it was


# ---------------------------------------------------------------------------------------------------------------------------------
# the pixel-side operators
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,patch", [(32, 8), (256, 8)])
def test_mask_tokens_and_composite_against_numpy(H, patch):
    B, Cn = 4, 3
    rng = np.random.default_rng(H)
    g = H // patch
    pix = np.zeros((B, H, H), dtype=np.uint8)
    pix[1] = 1                                                                     # image 0: all zero; image 1: all one
    for k, (dy, dx) in enumerate([(0, 0), (0, patch - 1), (patch - 1, 0), (patch - 1, patch - 1)]):
        r, c = (3 * k + 1) % g, (5 * k + 2) % g                                    # image 2: single lit pixels, one per patch corner
        pix[2, r * patch + dy, c * patch + dx] = 255
    pix[3] = (rng.random((H, H)) < 0.01) * rng.integers(1, 256, (H, H))            # image 3: scattered, any non-zero value
    ids_np = rng.integers(0, 50, (B, g * g)).astype(np.int64)
    want_ids, want_counts = mask_tokens_np(pix, patch, ids_np, MASK_ID)
    ids, counts = ops.mask_tokens(t(pix), patch, t(ids_np), MASK_ID)
    assert np.array_equal(n(ids), want_ids) and np.array_equal(n(counts), want_counts)
    assert want_counts[0] == 0 and want_counts[1] == g * g and want_counts[2] == 4 and 4 < want_counts[3] < g * g
    gen = rng.standard_normal((B, Cn, H, H)).astype(np.float32)
    orig = rng.standard_normal((B, Cn, H, H)).astype(np.float32)
    gen[0, 0, 0, 0], orig[1, 0, 0, 0] = np.nan, np.nan                             # the side that is not taken never reaches the result
    want = composite_np(gen, orig, pix)
    assert np.isfinite(want).all()
    assert np.array_equal(n(ops.composite(t(gen), t(orig), t(pix))), want)
    g_dev = t(gen)
    out = ops.composite(g_dev, t(orig), t(pix), out=g_dev)                         # out aliases gen
    assert out.data_ptr() == g_dev.data_ptr() and np.array_equal(n(g_dev), want)


# ---------------------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------------------
def _start(pipe, areas, seed):
    """encoded ids of B random images with areas[b] random positions masked -> (ids, counts)"""
    B, N = len(areas), pipe.num_tokens
    g = torch.Generator().manual_seed(seed)
    img = (torch.rand(B, 3, pipe.image_size, pipe.image_size, generator=g) * 2 - 1).to(dev())
    ids = pipe.to_latent(img)[1].reshape(B, N).clone()
    for b, m in enumerate(areas):
        ids[b, torch.randperm(N, generator=g)[:m].to(dev())] = pipe.mask_token_id
    return ids, list(areas)


def _opts(pipe, ctx, B, T, topk=5, top_p=None, guidance_scale=None, context_lens=None, choice_temperature=None, negative=None, negative_lens=None):
    return pipe._options(topk, top_p, guidance_scale, context_lens, choice_temperature, ctx, B, negative, negative_lens, T)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_native_loop_equals_the_composition_and_one_graph_serves_every_mask(tiny, dtype):
    pipe = tiny
    B, seed = 3, 41
    try:
        pipe.set_compute_dtype(dtype)
        for text in (None, ["a", "b", "c"]):
            ctx = None if text is None else pipe.text_model(text)
            for T in (1, 3, 8):
                opts = _opts(pipe, ctx, B, T)
                first = _start(pipe, (0, 5, 16), seed=T)
                second = _start(pipe, (1, 2, 16), seed=T + 100)
                want = [composed_edit(pipe, ids, counts, ctx, T, 1.0, opts, seed, image_base=2) for ids, counts in (first, second)]
                assert not torch.equal(want[0][0], want[1][0])
                for (ids0, counts), (want_ids, want_img) in zip((first, second), want):
                    assert not bool((want_ids == pipe.mask_token_id).any())
                    keep = ids0 != pipe.mask_token_id
                    assert torch.equal(want_ids[keep], ids0[keep])
                    ids, img = pipe.edit_ids(ids0, counts, ctx, T, 1.0, opts, seed, image_base=2, use_graph=False)
                    assert torch.equal(ids, want_ids) and torch.equal(img, want_img), (dtype, text, T, "eager")
                # the graph: warm-up (eager), capture, replay -- then the OTHER masks through the same graph: the table is read, not baked in
                for which in (0, 0, 0, 1, 0):
                    ids0, counts = (first, second)[which]
                    ids, img = pipe.edit_ids(ids0, counts, ctx, T, 1.0, opts, seed, image_base=2, use_graph=True)
                    assert torch.equal(ids, want[which][0]) and torch.equal(img, want[which][1]), (dtype, text, T, "graph", which)
    finally:
        pipe.set_compute_dtype(torch.float32)


def test_options_compose(tiny):
    pipe = tiny
    B, T, seed = 3, 3, 9
    texts, negs = ["a", "b", "c"], ["not x", "not y", "not z"]
    ctx, ctx_lens = pipe.text_model(texts, return_lens=True)
    neg, neg_lens = pipe.text_model(negs, return_lens=True)
    ids0, counts = _start(pipe, (3, 9, 16), seed=5)
    cases = (dict(guidance_scale=3.0),
             dict(guidance_scale=[0.5, 3.0, 1.25], negative=neg, negative_lens=neg_lens),
             dict(context_lens=ctx_lens),
             dict(choice_temperature=4.5),
             dict(topk=None, top_p=0.9))
    results = []
    for kw in cases:
        opts = _opts(pipe, ctx, B, T, **kw)
        want_ids, want_img = composed_edit(pipe, ids0, counts, ctx, T, 1.0, opts, seed)
        for use_graph in (False, True, True, True):
            ids, img = pipe.edit_ids(ids0, counts, ctx, T, 1.0, opts, seed, use_graph=use_graph)
            assert torch.equal(ids, want_ids) and torch.equal(img, want_img), (kw.keys(), use_graph)
        results.append(want_ids)
    plain = composed_edit(pipe, ids0, counts, ctx, T, 1.0, _opts(pipe, ctx, B, T), seed)[0]
    assert sum(not torch.equal(r, plain) for r in results) >= 3                    # the options are seen


def test_full_mask_ties_to_the_pinned_loop(tiny):
    """m = N: the edit schedule is loop_schedule's at every step but the last, where that loop re-masks one token and the edit none"""
    pipe = tiny
    B, T, N, seed = 2, 8, pipe.num_tokens, 17
    _, nmask, _ = loop_schedule(T, 1.0, N)
    sched = edit_schedule(N, T)
    assert sched[:-1] == nmask[:-1] and sched[-1] == 0 and nmask[-1] == 1
    img = (torch.rand(B, 3, pipe.image_size, pipe.image_size, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev())
    g = pipe.image_size // pipe.patch_size
    _, ids = pipe.edit(img, token_mask=torch.ones(g, g, dtype=torch.bool), timesteps=T, topk=5, seed=seed, return_ids=True)
    start = torch.full((B, N), pipe.mask_token_id, dtype=torch.long, device=dev())
    ref, _ = pipe.generate_ids(None, B, T, 1.0, 5, [False] * T, seed, use_graph=False, streams=1, ids0=start)
    last = ref == pipe.mask_token_id
    assert last.sum(1).tolist() == [1] * B
    assert torch.equal(ids[~last], ref[~last])
    assert bool(((ids[last] >= 0) & (ids[last] < pipe.mask_token_id)).all())


def test_invariants_at_full_size():
    pipe, _ = scaled_chain_pipeline()
    try:
        pipe.set_compute_dtype(torch.bfloat16)
        B, T, S, p = 2, 4, pipe.image_size, pipe.patch_size
        g = torch.Generator().manual_seed(2)
        img = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).to(dev())
        mask = torch.zeros(B, S, S, dtype=torch.uint8)
        mask[0, 37:150, 90:201] = 1                                                # a rectangle that cuts through patches
        mask[1] = (torch.rand(S, S, generator=g) < 0.002).to(torch.uint8)          # a scattered set
        enc = pipe.to_latent(img)[1].reshape(B, -1)
        out, ids = pipe.edit(img, mask=mask, timesteps=T, seed=3, preserve="pixels", return_ids=True)
        tm = (mask.reshape(B, S // p, p, S // p, p).amax(dim=(2, 4)) != 0).reshape(B, -1).to(dev())
        assert 0 < int(tm[1].sum()) < tm.shape[1] and int(tm[0].sum()) == (19 - 4) * (26 - 11)
        assert torch.equal(ids[~tm], enc[~tm])
        assert not bool((ids == pipe.mask_token_id).any())
        sel = (mask != 0)[:, None].expand_as(img).to(dev())
        assert torch.equal(out[~sel], img[~sel]) and bool(torch.isfinite(out).all())
    finally:
        pipe.set_compute_dtype(torch.float32)
