"""Per-image context lengths at the model level (the *_lens entries of include/pmhip.h) on the tiny pipeline, fp32-verify and bf16,
B = 4, L = 77, lengths (1, 33, 64, 77): context rows at or beyond an image's length never reach a result (NaN included), the
default is untouched, an image does not see its neighbours' lengths, one captured graph serves every mix of lengths, the result
is that of the truncated context, and a decode session serves contexts of different lengths bit for bit like the batch loop."""
import pytest
import torch

import paintmind_amd as pm
from gpu_common import dev
from paintmind_amd.generate import Pipeline, mask_schedule, num_token_masked
from util import load_golden, to_torch_sd

pytestmark = pytest.mark.gpu

TOL = 1e-3                      # the project's float bar (tests/test_gpu_slots.py, tests/test_gpu_model.py)
L, LENS = 77, (1, 33, 64, 77)
B = len(LENS)
T, TOPK, TEMP, SEED = 5, 4, 1.0, 77
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


@pytest.fixture(scope="module")
def tiny_pipe():
    p, _ = load_golden("tiny_pipeline.npz")
    pipe = Pipeline(pm.Config(pm.ver2cfg["tiny-pipeline"]), stage1_pretrained=False)
    missing = pipe.load_state_dict(to_torch_sd(p), strict=False)
    assert not missing.unexpected_keys and all(k.startswith("text_model") for k in missing.missing_keys)
    return pipe.to(dev()).eval()


@pytest.fixture(scope="module")
def data(tiny_pipe):
    pipe = tiny_pipe
    g = torch.Generator().manual_seed(11)
    ctx = pipe.text_model(["w", "x", "y", "z"]).to(dev())
    ids = torch.randint(0, pipe.mask_token_id, (B, pipe.num_tokens), generator=g)
    ids[torch.rand(B, pipe.num_tokens, generator=g) < 0.5] = pipe.mask_token_id
    ids = ids.to(dev())
    fills = {"zeros": lambda r, d: torch.zeros(r, d), "large": lambda r, d: 50 * torch.randn(r, d, generator=g),
             "nan": lambda r, d: torch.full((r, d), float("nan"))}

    def padded(name, lens=LENS):
        c = ctx.clone()
        for b, m in enumerate(lens):
            c[b, m:] = fills[name](L - m, c.shape[2]).to(dev())
        return c
    return dict(ctx=ctx, ids=ids, tok=pipe.ids2tokens(ids), padded=padded)


class in_dtype:
    def __init__(self, pipe, dtype):
        self.pipe, self.dtype = pipe, dtype

    def __enter__(self):
        self.pipe.set_compute_dtype(self.dtype)

    def __exit__(self, *exc):
        self.pipe.set_compute_dtype(torch.float32)


def steps(pipe, ctx, lens, scale=None, batch=B, image_base=0, T=T, topk=TOPK, temperature=TEMP, seed=SEED):
    """the decode loop step by step through the scalar one-step entry -> (final ids, [pred per step], [score per step])"""
    eng = pipe.engine()
    temps, nmask = pipe._schedule(T, temperature)
    ids = torch.full((batch, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
    preds, scores = [], []
    for step in range(T):
        ids, _, pred, score = eng.sample(None, ids, ctx, topk, temps[step], nmask[step], seed=seed, step=step, image_base=image_base,
                                         want_img=False, want_aux=True, guidance_scale=scale, context_lens=lens)
        preds.append(pred.clone())
        scores.append(score.clone())
    return ids, preds, scores


def loop(pipe, ctx, lens, **kw):
    kw = {**dict(use_graph=False, streams=1), **kw}
    return pipe.generate_ids(ctx, B, T, TEMP, TOPK, [False] * (T - 1) + [True], SEED, context_lens=lens, **kw)


@DTYPES
def test_padding_rows_never_reach_a_result(tiny_pipe, data, dtype):
    """zeros, 50 * randn or NaN behind every image's length: the same logits, per-step predictions and scores, ids and image"""
    pipe = tiny_pipe
    with in_dtype(pipe, dtype):
        ref = None
        for name in ("zeros", "large", "nan"):
            ctx = data["padded"](name)
            got = (pipe.tokens2logits(data["tok"], ctx, context_lens=list(LENS)),) + steps(pipe, ctx, list(LENS)) + loop(pipe, ctx, list(LENS))
            logits, ids, preds, scores, loop_ids, imgs = got
            assert torch.isfinite(logits).all() and torch.isfinite(imgs).all() and all(torch.isfinite(s).all() for s in scores), name
            assert torch.equal(ids, loop_ids), name                 # the loop entry and the step entry agree
            flat = [logits, ids, *preds, *scores, loop_ids, imgs]
            if ref is None:
                ref = flat
            assert all(torch.equal(a, b) for a, b in zip(flat, ref)), name


@DTYPES
def test_full_lengths_are_the_entries_without_lengths(tiny_pipe, data, dtype):
    pipe, ctx, full = tiny_pipe, data["ctx"], [L] * B
    with in_dtype(pipe, dtype):
        assert torch.equal(pipe.tokens2logits(data["tok"], ctx, context_lens=full), pipe.tokens2logits(data["tok"], ctx))
        for scale in (None, 2.0):
            a = pipe.sample(data["ids"], 0.5, text=ctx, topk=3, temperature=0.8, seed=5, guidance_scale=scale, context_lens=full)
            b = pipe.sample(data["ids"], 0.5, text=ctx, topk=3, temperature=0.8, seed=5, guidance_scale=scale)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), scale
            for use_graph in (False, True, True):
                x = loop(pipe, ctx, full, use_graph=use_graph, guidance_scale=scale)
                y = loop(pipe, ctx, None, use_graph=use_graph, guidance_scale=scale)
                assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]), (scale, use_graph)
        # a device tensor of lengths is as good as a list
        assert torch.equal(pipe.tokens2logits(data["tok"], ctx, context_lens=torch.tensor(LENS, device=dev())),
                           pipe.tokens2logits(data["tok"], ctx, context_lens=list(LENS)))


@DTYPES
def test_an_image_does_not_see_its_neighbours_lengths(tiny_pipe, data, dtype):
    pipe, ctx = tiny_pipe, data["padded"]("nan")
    with in_dtype(pipe, dtype):
        base_logits = pipe.tokens2logits(data["tok"], ctx, context_lens=list(LENS))
        base_ids, base_preds, base_scores = steps(pipe, ctx, list(LENS))
        for others in (1, 20):
            for j in range(B):
                lens = [min(others, LENS[b]) for b in range(B)]       # never beyond an image's finite rows
                lens[j] = LENS[j]
                assert torch.equal(pipe.tokens2logits(data["tok"], ctx, context_lens=lens)[j], base_logits[j]), (others, j)
                ids, preds, scores = steps(pipe, ctx, lens)
                assert torch.equal(ids[j], base_ids[j]), (others, j)
                assert all(torch.equal(a[j], b[j]) for a, b in zip(preds + scores, base_preds + base_scores)), (others, j)


@DTYPES
def test_one_graph_serves_every_mix_of_lengths(tiny_pipe, data, dtype):
    pipe, ctx = tiny_pipe, data["padded"]("nan")
    with in_dtype(pipe, dtype):
        for scale in (None, 2.5):
            eager = loop(pipe, ctx, list(LENS), guidance_scale=scale)
            ids_s, _, _ = steps(pipe, ctx, list(LENS), scale=scale)
            assert torch.equal(eager[0], ids_s), scale
            for _ in range(3):                                        # first call eager, second captures, third replays
                got = loop(pipe, ctx, list(LENS), use_graph=True, guidance_scale=scale)
                assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1]), scale
            other = [1, 7, 40, 64]                                    # a replay with lengths the capture never saw
            want = loop(pipe, ctx, other, guidance_scale=scale)
            got = loop(pipe, ctx, other, use_graph=True, guidance_scale=scale)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), scale
            assert not torch.equal(want[0], eager[0])
            for use_graph in (False, True, True):                     # two lanes: every micro-batch takes its slice of the lengths
                got = loop(pipe, ctx, list(LENS), use_graph=use_graph, streams=2, guidance_scale=scale)
                assert torch.equal(got[0], eager[0]) and torch.equal(got[1], eager[1]), (scale, use_graph)


@DTYPES
def test_guided_step_and_loop_with_lengths_equal_the_operator_composition(tiny_pipe, data, dtype):
    """as tests/test_gpu_model.py does without lengths: pmhip_s2_forward_lens + pmhip_s2_forward + pmhip_guidance_combine + the
    sampling operators, step by step, against the native guided step and the native guided loop"""
    pipe, ctx, scale = tiny_pipe, data["padded"]("nan"), 2.5
    with in_dtype(pipe, dtype):
        ids = torch.full((B, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
        ref = []
        for step in range(T):
            nm = num_token_masked(mask_schedule((step + 1) / T), pipe.num_tokens)
            temp = TEMP * (1 - step / T)
            one_ids, one_img = pipe.sample(ids, mask_schedule((step + 1) / T), text=ctx, topk=TOPK, temperature=temp, seed=SEED, step=step,
                                           guidance_scale=scale, context_lens=list(LENS))
            ids, img = pipe._sample_guided_composed(ids, nm, ctx, TOPK, temp, None, SEED, step, 0, scale, context_lens=list(LENS))
            assert torch.equal(one_ids, ids) and torch.equal(one_img, img), step
            ref.append(img)
        for use_graph in (False, True, True):
            gids, imgs = pipe.generate_ids(ctx, B, T, TEMP, TOPK, [True] * T, SEED, use_graph=use_graph, streams=1, guidance_scale=scale,
                                           context_lens=list(LENS))
            assert torch.equal(gids, ids) and all(torch.equal(a, b) for a, b in zip(imgs, ref)), use_graph


@DTYPES
def test_lengths_against_the_truncated_context(tiny_pipe, data, dtype):
    """Image b with (context, len_b) against the same image with its context CUT to len_b rows, run at the same B.  The two differ
    in the shape of the context GEMMs (M = B * len_b rows instead of B * L) and of the cross-attention launch, not in the
    arithmetic a row asks for; whether the small-M GEMMs take the same kernel has not been measured (DESIGN.md section 4l
    records the figures once they are).  fp32-verify is gated at the project's float bar; the bf16 figure is printed, not gated.  Counter-check: WITHOUT lengths, padding rows of 50 * randn move the logits far beyond the bar, so this
    test cannot pass with the lengths ignored."""
    pipe, tok = tiny_pipe, data["tok"]
    with in_dtype(pipe, dtype):
        masked = pipe.tokens2logits(tok, data["padded"]("nan"), context_lens=list(LENS))
        loud = pipe.tokens2logits(tok, data["padded"]("large"))
        worst, gap = 0.0, 0.0
        for b, m in enumerate(LENS):
            cut = pipe.tokens2logits(tok, data["ctx"][b:b + 1, :m].expand(B, m, -1).contiguous())[b]
            worst = max(worst, float((masked[b] - cut).abs().max()))
            if m < L:
                gap = max(gap, float((loud[b] - cut).abs().max()))
        print(f"{dtype}: max |logits(context, lens) - logits(truncated context)| = {worst:.3e}; padding of 50 * randn without lengths: {gap:.3e}")
        if dtype == torch.float32:
            assert worst < TOL
        assert gap > 100 * TOL


def test_length_validation(tiny_pipe, data):
    pipe, ctx = tiny_pipe, data["ctx"]
    from paintmind_amd import _lib
    for bad in ([0, 5, 5, 5], [5, 5, 5, L + 1], [5, 5, 5]):
        for call in (lambda: pipe.tokens2logits(data["tok"], ctx, context_lens=bad), lambda: loop(pipe, ctx, bad),
                     lambda: pipe.sample(data["ids"], 0.5, text=ctx, context_lens=bad)):
            with pytest.raises((ValueError, _lib.PmhipError)):
                call()
    with pytest.raises(ValueError):
        loop(pipe, None, [1, 1, 1, 1])


# ------------------------------------------------------------------------------------------------------------------------------
# sessions: requests whose contexts have different lengths
# ------------------------------------------------------------------------------------------------------------------------------
# tick -> [(context rows, T, temperature, topk, seed, image index, guidance scale)], admitted staggered into 3 slots
PLAN = {0: [(33, 6, 1.0, 5, 101, 3, None), (1, 2, 0.7, 1, 102, 9, 2.0)],
        1: [(64, 4, 1.3, 3, 103, 4, None)],
        3: [(77, 5, 0.0, 4, 104, 30, 1.5), (33, 2, 0.9, 2, 105, 5, None)],
        6: [(1, 4, 1.0, 5, 106, 2 ** 33 + 1, None), (64, 3, 0.5, 2, 107, 8, 3.0)]}
S = 3


def run_session(pipe, use_graph, max_context_len, contexts):
    s = pipe.decode_session(slots=S, conditional=True, use_graph=use_graph, record_steps=True, decode=False, max_context_len=max_context_len)
    out, tick, number, caps = [], 0, 0, []
    while tick <= max(PLAN) or not s.idle():
        for req in PLAN.get(tick, []):
            h = s.submit(context=contexts[number][:req[0]], timesteps=req[1], temperature=req[2], topk=req[3], seed=req[4], image_index=req[5],
                         guidance_scale=req[6])
            h.params, h.full = req, contexts[number]
            number += 1
        out += s.step()
        caps.append(s._ctx.shape[1])
        tick += 1
    assert s.idle() and len(out) == number == 7
    return out, caps


def reference(pipe, j, req, full, caps):
    """row j of the scalar path at B = S with the request's context padded (zeros) to the session's capacity and its length in row
    j.  caps[t] = the capacity in force at the request's step t: per-step pred / score and the ids come from the scalar one-step
    entry run at that capacity; where the capacity never moved the ids must also end where generate_ids (eager, one stream) ends"""
    m, T_, temp, topk, seed, k, scale = req
    eng = pipe.engine()
    temps, nmask = pipe._schedule(T_, temp)
    ids = torch.full((S, pipe.num_tokens), pipe.mask_token_id, dtype=torch.long, device=dev())
    preds, scores = [], []
    for step, cap in enumerate(caps):
        ctx = torch.zeros(S, cap, full.shape[1], device=dev())
        ctx[j, :m] = full[:m]
        lens = [cap] * S
        lens[j] = m
        ids, _, pred, score = eng.sample(None, ids, ctx, topk, temps[step], nmask[step], seed=seed, step=step, image_base=k - j,
                                         want_img=False, want_aux=True, guidance_scale=scale, context_lens=lens)
        preds.append(pred[j].clone())
        scores.append(score[j].clone())
    if len(set(caps)) == 1:
        ids_loop, _ = pipe.generate_ids(ctx, S, T_, temp, topk, [False] * T_, seed, image_base=k - j, use_graph=False, streams=1,
                                        guidance_scale=scale, context_lens=lens)
        assert torch.equal(ids, ids_loop)
    return ids[j].clone(), preds, scores


@DTYPES
def test_sessions_serve_contexts_of_different_lengths(tiny_pipe, dtype):
    """Fixed capacity: eager, the first graph call, capture, replay.  Then a capacity that grows with the contexts admitted -- 33
    rows at tick 0, 64 at tick 1, 77 at tick 3 -- while requests are under way: a step at capacity C is the scalar step at
    capacity C (growing re-prepares the context at another GEMM shape, so the reference follows the capacity step by step)."""
    pipe = tiny_pipe
    contexts = list(pipe.text_model([f"p{i}" for i in range(7)]).to(dev()))
    refs = {}
    with in_dtype(pipe, dtype):
        for use_graph, cap in ((False, L), (True, L), (True, L), (True, L), (False, None), (True, None)):
            done, caps = run_session(pipe, use_graph, cap, contexts)
            assert caps[:4] == ([L] * 4 if cap else [33, 64, 64, 77]) and caps[-1] == L
            for f in done:
                h = f.handle
                step_caps = tuple(caps[h.admitted:h.admitted + h.timesteps])
                key = (h.params, h.slot, step_caps)
                if key not in refs:
                    refs[key] = reference(pipe, h.slot, h.params, h.full, step_caps)
                ids_ref, preds, scores = refs[key]
                assert len(h.trace) == h.timesteps == len(step_caps)
                for step in range(h.timesteps):
                    assert torch.equal(h.trace[step][0], preds[step]), (use_graph, cap, h.params, h.slot, step, "pred")
                    assert torch.equal(h.trace[step][1], scores[step]), (use_graph, cap, h.params, h.slot, step, "score")
                assert torch.equal(f.ids, ids_ref), (use_graph, cap, h.params, h.slot)


def test_session_context_shapes(tiny_pipe):
    pipe = tiny_pipe
    s = pipe.decode_session(slots=2, conditional=True, max_context_len=40, decode=False)
    with pytest.raises(ValueError, match="max_context_len"):
        s.submit(context=torch.zeros(41, 96))
    s.submit(context=torch.randn(40, 96), timesteps=2)
    s.submit(context=torch.randn(7, 95), timesteps=2)                 # the width stays one per session
    with pytest.raises(ValueError, match="width"):
        s.step()
